// af_api.cpp -- the C ABI of include/audioforge_mi.h on top of the host mirror and the kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "af_api_internal.hpp"
#include "af_device.h"
#include "af_host.hpp"
#include "af_mixdown_host.hpp"
#include "af_output_writer_host.hpp"
#include "af_resampler_host.hpp"
#include "af_retune.h"
#include "af_stages.h"
#include "af_stream_state_host.hpp"
#include "af_suppressor_host.hpp"
#include "af_switches.hpp"

namespace af {
size_t lane_kernel_dynamic_lds(int lookahead_samples);
hipError_t launch_chain_lane(const LaunchArgs &args, int lookahead_samples, hipStream_t stream);
size_t ring_kernel_dynamic_lds(int n_sections, int lookahead_samples, bool crossfade);
hipError_t launch_chain_ring(const LaunchArgs &args, int n_sections, int lookahead_samples, bool crossfade, int variant,
                             bool auto_makeup, hipStream_t stream);
hipError_t launch_chain_ring_lds(const LaunchArgs &args, size_t dyn, int variant, bool auto_makeup, hipStream_t stream);
hipError_t launch_chain_publish_ready(int64_t *ready, int64_t samples, hipStream_t stream);
hipError_t launch_chain_quad(const LaunchArgs &args, int n_sections, int lookahead_samples, bool crossfade, int waves,
                             hipStream_t stream);
size_t quad_kernel_dynamic_lds(int n_sections, int lookahead_samples, bool crossfade);
hipError_t launch_merge_side_stats(BlockStats *rows, const BlockStats *input_rows, const BlockStats *deesser_rows,
                                   int64_t n, hipStream_t stream);
hipError_t launch_deesser(const ChainParams *d_params, double *st64, float *st32, const float *in, float *out,
                          BlockStats *rows, int64_t n_samples, int64_t stream_stride, int32_t n_streams,
                          int32_t layout, bool front_end, bool write_out_power, hipStream_t stream);
hipError_t launch_eq_systolic(const ChainParams *d_params, const int32_t *d_group_preset, double *st64, const float *in, float *audio,
                              float *ring, float *ring_in, int32_t ring_rows, int64_t n0, BlockStats *stats, bool crossfade,
                              int64_t n_samples, int64_t stream_stride, int32_t n_streams, hipStream_t stream,
                              double *block_power = nullptr, int n_sections = -1);
bool comp_roles_serves(const ChainParams &p);
bool lim_roles_serves(const ChainParams &p);
hipError_t launch_chain_comp_roles(const LaunchArgs &args, bool sidechain, bool adaptive, hipStream_t stream);
hipError_t launch_chain_lim_roles(const LaunchArgs &args, int max_lookahead, hipStream_t stream);
constexpr size_t kMaxLdsBytes = 160 * 1024;
}  // namespace af

// AUTO routes the configurations the stage pipeline serves to it up to this many streams.  Measured (dynamics chain, 10 s,
// one MI355X): 256 streams 41 ms against the token ring's 202, 1024 streams 64, 2048 streams 91, 3072 streams 136, 4096
// streams 202 (the hand-over rings cost 0.3 KB per sample step per stream: the HBM roof); beyond that the token ring wins
// (a launch of it lasts ~202 ms up to 16 384 streams).  Behind the suppressor, whose kernels use the same HBM, up to 2048.
constexpr int kStagedAutoMaxStreams = 3072, kStagedAutoMaxStreamsBehindSuppressor = 2048;
constexpr int kEqParamSlots = 16;  // parameter blocks the EQ / de-esser stages read: one per window in flight (af_engine::d_params_eq)

static_assert(sizeof(af_block_stats) == sizeof(af::BlockStats), "stats row layout");
static_assert(sizeof(af_block_stats) == 72, "stats row size");

thread_local std::string af_last_error_text;

// one chain preset of an engine: the prototype the setters edit and its flattened parameter block (export_params)
struct af_preset {
  af::ChainProto proto;
  af::ChainParams params{};
  explicit af_preset(double fs) : proto(fs) {}
};

struct af_engine {
  // Presets.  An engine is N streams in groups of 64 (one chain workgroup each); every group runs one preset.  The table is
  // never empty: af_engine_set_preset_count adds fresh ones (and reallocates: base() and selected() are taken fresh at each
  // use), the setters address the selected one, af_engine_assign_presets maps groups to presets.  The device holds the
  // parameter blocks as an array and, with more than one preset, a group -> preset table.
  std::vector<af_preset> presets;
  int current_preset = 0;
  int n_presets() const { return (int)presets.size(); }
  af_preset &base() { return presets[0]; }  // preset 0: what decides everything the presets must agree on
  const af_preset &base() const { return presets[0]; }
  af_preset &selected() { return presets[(size_t)current_preset]; }
  const af_preset &selected() const { return presets[(size_t)current_preset]; }
  std::vector<int32_t> group_preset;         // [ceil(n_streams / 64)], empty = every group runs preset 0
  af::DeviceBuffer<int32_t> d_group_preset;
  // The parameter blocks on the device, each beside a host copy of what it holds: a launch site hands over the blocks it is
  // about to run on and only a change is uploaded (first launch; while a coefficient crossfade advances; a live setter).
  // af_engine_reset invalidates all four.
  af::Mirrored<af::ChainParams> d_params;      // [n_presets()]: what the chain kernels and the stage kernels read
  af::Mirrored<af::ChainParams> d_params_pre;  // the pre-pass launch's variant (auto-makeup, EQ-before-de-esser)
  af::Mirrored<af::ChainParams> d_params_de;   // the de-esser pass reads the unedited parameter block
  af::Mirrored<af::ChainParams> d_params_eq;   // [kEqParamSlots][n_presets()]: what the systolic EQ kernel reads (af_eq_systolic.hip)
  uint64_t eq_slot_cursor = 0;               // stage pipeline with the de-esser: the next window's parameter slot
  int n_streams;
  int device;
  bool touched_device = false;  // use_device() succeeded once: there may be allocations, and the destructor has a device to wait for
  bool started = false;
  bool params_dirty = true;
  int kernel = AF_KERNEL_AUTO;
  int ring_variant = 0;
  bool timing = false;
  int64_t samples_processed = 0;
  int64_t last_blocks = 0;
  double last_kernel_ms = 0.0;
  int last_launches = 0;
  int last_kernel_used = 0;  // AF_KERNEL_* of the most recent chain launch

  af::DeviceBuffer<double> d_st64;
  af::DeviceBuffer<float> d_st32;
  int n_f64 = 0, n_f32 = 0;
  af::DeviceBuffer<af::BlockStats> d_stats;
  af::DeviceBuffer<af::BlockStats> d_stats_pre;  // rows of the pre-pass launch (auto-makeup)
  af::DeviceBuffer<double> d_block_power;  // [blocks][streams] of the current call: compressor-input block power written by the systolic EQ
  // Parameter uploads go through engine-owned pinned staging slots: the host never waits for a stream, and a slot is only
  // reused once the copy that read it has run.
  af::PinnedSlots<32> stager;  // (the stage pipeline with the de-esser uploads one block per window: the host may run this many windows ahead)
  // Device buffers that had to grow while earlier work may still read them: kept until that work has ended (an event on the
  // stream the call was made on), freed by a later call, a reset or the destructor -- growing never synchronises the device.
  af::RetireList retired;
  // The side streams (ensure_side_streams): owned, or under AF_SERIAL_STREAMS aliases of the caller's stream.
  af::Stream syn_stream;                   // CU partition: pitch spectra + network + resynthesis (else the caller's stream)
  af::Stream fin_stream;                   // resynthesis + overlap-add of window w beside pitch spectra + network of w+1
  af::Stream lim_stream;                   // AF_ROLES=2: the limiter half of the chain (af_roles.hip) on CUs of its own
  af::Stream eq_stream;                    // the window's systolic EQ (af_eq_systolic.hip), behind its overlap-add, beside the next window's synthesis
  int partition_chain_cus = 0;             // CUs reserved for the chain stream (0 = the streams are not masked)
  af::DeviceBuffer<af::BlockStats> d_stats_de;    // rows of the de-esser pass
  af::DeviceBuffer<double> d_vad;          // [blocks][streams] speech posteriors for the next call
  int64_t vad_blocks = 0;
  double vad_reliability = 0.0, noise_floor_db = 0.0, live_noise_reliability = 0.0;
  bool has_evidence = false;
  af::DeviceBuffer<int32_t> d_status;
  af::DeviceBuffer<int64_t> d_ready;         // samples of the running call the suppressor's side has finished (LaunchArgs::ready)
  af::DeviceBuffer<float> d_io;  // staging for the host entry point
  hipStream_t last_stream = nullptr;
  af::SuppressorHost supp;
  af::Stream aux_stream;                                 // chain launches while the suppressor fills the chip
  af::Stream pre_stream;                                 // the suppressor's sample-serial pre-pass, two windows ahead
  af::Stream ana_stream;                                 // spectra + pitch, one window ahead
  std::vector<af::Event> sync_events;
  size_t ev_cursor = 0;                                  // next free entry of sync_events within the current call
  std::vector<af::TimedSpan> chain_ms_events;  // timing brackets of the chain launches of the last call
  // rnnoise.rs:114-164: the samples of a call that do not fill a 480-sample frame wait here for the next call
  af::DeviceBuffer<float> d_pending;  // [streams][480]
  int pending = 0;              // samples per stream waiting in d_pending (all streams advance in lock step)
  af::DeviceBuffer<float> d_asm;  // [streams][asm_stride]: pending samples + this call's, when the two have to be joined
  int64_t last_output_samples = 0;  // samples per stream the last process call produced
  af::DeviceBuffer<int32_t> d_trace;  // [frames][streams][2]: (silence, pitch index) of every frame of the last call
  int64_t trace_frames = 0;
  bool trace = false;
  // the stage-pipeline form of the chain (af_stages.hip): rings, one stream and a ring of events per stage
  struct StagePipe {
    bool decided = false, active = false;  // chosen at the first call after a reset, then kept (the rings ARE the histories)
    af::StageRings rings{};
    std::vector<af::DeviceBuffer<>> allocs;
    int64_t tw_max = 0;                    // longest window the rings were sized for
    af::Stream stream;                     // where the launch steps go when the suppressor's pipeline feeds the chain
    int64_t windows = 0;                   // windows launched since the rings were last cleared
    static constexpr int kMkSets = 4;
    af::DeviceBuffer<double> d_mk;
    int64_t mk_rows = 0;                   // rows (blocks x streams) per set
    static constexpr int kBpSets = 16;
    af::DeviceBuffer<double> d_bp;         // auto-makeup: block powers, written seven launch steps before they are read
    int64_t call_stride = 0;               // stream stride of the call being scheduled
    bool with_deesser = false;             // the rings include the de-esser stages'
    int32_t w_min = 1;                     // smallest lookahead + 1 over the presets
    uint32_t strip = 0;                    // chain flags another kernel has taken over (the suppressor's pre-pass)
  } pipe;
  // measured 12..80 (AF_SUPP_WINDOW_FRAMES).  Round 1 (one chain launch per window): 20 -> 248 ms per bench step, 24 -> 252, 30 ->
  // 254, 16 -> 259, 50 -> 260.  End of round 3 (one chain launch per call: a window costs the chain nothing any more):
  // 12 -> 165.2, 14 -> 166.1, 16 -> 163.2, 18 -> 164.5, 20 -> 165.0, 24 -> 166.7, 32 -> 169.2
  int supp_window_frames = 16;
  af::Event ev_start, ev_stop, ev_mid;  // start | suppressor done | chain done
  // the noise gate stage (realtime stage 1, dsp_loop.rs:1371-1435): engine-wide parameters, live between calls; per-stream
  // state in `d_gate` ([af::kGateFields][stream], zero = NoiseGate's initial state), allocated at the first gated call and
  // touched only by the pre-pass that gates
  bool gate_enabled = false;
  double gate_threshold_db = -40.0, gate_attack_ms = 10.0, gate_release_ms = 100.0;  // NoiseGate::new(-40, 10, 100, fs)
  int gate_mode = 0;                 // 0 ThresholdOnly, 1 VadAssisted, 2 VadOnly
  af::DeviceBuffer<int64_t> d_gate;
  // the VAD-fused modes (gate.rs:652-741): a VadAutoGate::without_backend attached to the gate.  Its settings are engine-wide
  // and kept across a detach; its state and the fused gate's own fields live in `d_gate_vad` ([af::kVadFields][stream],
  // allocated at the first fused call).  `vad_ctl_fresh` / `vad_fused_fresh`: that part of the plane has to be (re)initialised
  // before the next fused pass (attach, reset, first use).
  bool gate_vad_attached = false, vad_ctl_fresh = true, vad_fused_fresh = true;
  float vad_threshold = 0.48f;       // ControlState's default, processor/control.rs:89
  float vad_hold_ms = 200.0f, vad_margin_db = 10.0f;  // vad.rs:667, 675
  bool vad_auto_threshold = true;
  af::DeviceBuffer<uint32_t> d_gate_vad;
  af::DeviceBuffer<uint32_t> d_vad_dec;  // [block][af::kVadDecWords][stream] decision rows of the running call
  int64_t vad_dec_blocks = 0;        // rows the last fused call wrote (af_engine_read_gate_vad_decisions)
  // evidence for the next fused call: one probability and one availability flag per control block, shared or per stream
  std::vector<float> vad_ev_prob;
  std::vector<uint8_t> vad_ev_avail;
  int64_t vad_ev_blocks = 0;
  bool vad_ev_per_stream = false;
  af::DeviceBuffer<uint8_t> d_vad_ev;  // [probabilities f32 | flags u8] of the running call
  af::PinnedSlots<8> ev_stager;      // it travels through pinned slots, as the parameter blocks do
  double sample_rate;
  // Device-rate I/O (dsp_loop.rs:274-317): a streaming product resampler in front of and / or behind the chain, built by
  // af_engine_set_io_sample_rates.  Null = that side runs at the engine's rate; both null = the engine as it always was.
  af_stream_resampler *rs_in = nullptr, *rs_out = nullptr;
  af::DeviceBuffer<float> d_rs_in, d_rs_mid, d_rs_out;  // af_engine_stream_host: device-rate input | engine-rate audio | device-rate output
  af_mixdown *mix = nullptr;     // af_engine_set_input_channels with more than one channel: the mixdown in front of everything
  af::DeviceBuffer<float> d_mix_in;  // af_engine_stream_host: the interleaved device frames
  // af_engine_set_output_writer: the output writer (output_writer.rs:62-343) behind the chain / the output resampler, at the
  // I/O output rate if one is set, otherwise at the engine's.  Null = off, every call is as without the setter.
  af_output_writer *ow = nullptr;
  uint32_t io_output_rate = 0;        // af_engine_set_io_sample_rates' output rate while it differs from the engine's
  std::vector<int64_t> ow_fill;       // af_engine_set_output_queue_fill; empty = the target centre (no error)
  std::vector<int64_t> ow_written;    // of the last af_engine_stream_host
  af::DeviceBuffer<int64_t> d_ow_fill, d_ow_written;
  af::DeviceBuffer<float> d_ow_out;
  int64_t ow_target_center = 0, ow_capacity = 0;
  bool ow_fill_dirty = true;          // the device copy of ow_fill is stale
  // Live control (af_engine_set_live_control): with the switch on the chain setters are accepted after streaming started.  A
  // setter then edits the prototype and this preset's parameter block (the next call uploads what changed, as it does while a
  // crossfade advances) and records what the reference setter does to the running object's STATE as edits of state-plane rows;
  // the next call that runs the chain applies the list with one launch of retune_state_kernel ahead of everything else.
  bool live_control = false;
  std::vector<af::RetuneOp> retune_ops;
  std::vector<char> live_retuned;     // per preset: a live setter was accepted since the last reset (the prototype follows the device)
  std::vector<char> live_cuts;        // per preset: ... one that moved the de-esser's cut frequencies (DeEsserParams::dyn_pending_row is in force)
  int dyn_pending_row = 0;            // first of the 15 plane rows behind every kernel's own (allocated with live control on), or 0
  af::DeviceBuffer<af::ChainParams> d_retune;  // the op list on the device, in parameter-block units (it travels through the parameter stager)
  af::TimedSpan retune_span;          // around the last call's launch of the retune kernel, if it made one with timing on
  // Per-stream lifecycle (af_engine_set_stream_lifecycle): restart, export and import of single streams between calls
  // (af_stream_state.h).  With the switch on the engine never runs the stage pipeline, whose rings are the histories.
  af::sstate::Lifecycle life;

  af_engine(double fs, int n, int dev) : presets(1, af_preset(fs)), n_streams(n), device(dev), sample_rate(fs) {}
  ~af_engine();
  hipError_t use_device() {
    const hipError_t err = hipSetDevice(device);
    touched_device |= err == hipSuccess;
    return err;
  }
};

// The device comes to rest first; the streams and the sub-objects go with the engine's device current; then the members (the
// suppressor's buffers among them) release themselves.  An engine that never used its device makes no HIP call here (nor do its sub-objects).
af_engine::~af_engine() {
  if (touched_device) {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    for (af::Stream *st : {&pipe.stream, &lim_stream, &fin_stream, &eq_stream, &syn_stream, &aux_stream, &pre_stream, &ana_stream}) st->reset();
  }
  af_stream_resampler_destroy(rs_in);
  af_stream_resampler_destroy(rs_out);
  af_mixdown_destroy(mix);
  af_output_writer_destroy(ow);
}

namespace {

int require_config(af_engine *e) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (e->started) {
    if (e->live_control)
      return fail(AF_ERR_STATE, "configuration setter called after streaming started: it changes which kernels, stages or buffers are "
                                "resident and is out of scope of live control; call af_engine_reset first");
    return fail(AF_ERR_STATE, "setter called after streaming started; call af_engine_reset first");
  }
  e->params_dirty = true;
  return AF_OK;
}

int check_band(int32_t band) {
  if (band < 0 || band >= af::kNumBands) return fail(AF_ERR_INVALID_ARGUMENT, "band index %d out of range", band);
  return AF_OK;
}

af::EqBandConfig to_cfg(const af_eq_band_config &c) {
  return af::EqBandConfig{c.filter_type, c.frequency_hz, c.gain_db, c.q, c.slope_db_per_octave, c.enabled != 0};
}

// Flatten the prototype into ChainParams (uniform) ...
void export_params(af_engine *e, const af::ChainProto &p, af::ChainParams &o) {
  std::memset(&o, 0, sizeof o);
  uint32_t f = 0;
  if (p.deesser_enabled) f |= af::kFlagDeesser;
  if (p.eq_enabled) f |= af::kFlagEq;
  if (p.compressor_enabled) f |= af::kFlagCompressor;
  if (p.limiter_enabled) f |= af::kFlagLimiter;
  if (p.eq_before_deesser) f |= af::kFlagEqBeforeDeesser;
  if (p.input_scrub) f |= af::kFlagInputScrub;
  if (p.input_clamp) f |= af::kFlagInputClamp;
  if (p.dc_block) f |= af::kFlagDcBlock;
  if (p.pre_highpass) f |= af::kFlagPreHighpass;
  o.flags = f;
  o.control_block = p.control_block;
  o.pre_hp = af::rbj_coefficients(af::BiquadType::HighPass, 80.0, 0.0, 0.707, p.sample_rate);
  int n = 0;
  for (int b = 0; b < af::kNumBands; ++b)
    for (int s = 0; s < p.eq.bands[b].processing_sections; ++s) o.eq[n++] = p.eq.bands[b].sections[s].section();
  o.n_eq_sections = n;
  o.comp = p.compressor.params(p.control_block);
  o.comp.vad_reliability = e->vad_reliability;
  o.comp.noise_floor_db = e->noise_floor_db;
  o.comp.live_noise_reliability = e->live_noise_reliability;
  o.comp.has_evidence = e->has_evidence ? 1 : 0;
  o.lim = p.limiter.params();
  o.deesser = p.deesser.params();
  // block_processor.rs:150-151: the TP ceiling follows the limiter ceiling on every block
  af::TruePeakProto tp = p.tp_limiter;
  tp.set_ceiling_linear(std::pow(10.0f, (float)p.limiter.ceiling_db / 20.0f));
  o.tp.ceiling_linear = tp.ceiling_linear;
  o.tp.release_coeff = tp.release_coeff;
}
void export_params(af_engine *e) {
  for (af_preset &ps : e->presets) export_params(e, ps.proto, ps.params);
}
// The presets' parameter blocks as a launch runs them: `strip` = flags another kernel has taken care of (a pre-pass's front
// end), `add` = flags that tell the kernels so.
std::vector<af::ChainParams> run_params(const af_engine *e, uint32_t strip, uint32_t add = 0) {
  std::vector<af::ChainParams> runs;
  runs.reserve(e->presets.size());
  for (const af_preset &ps : e->presets) {
    runs.push_back(ps.params);
    runs.back().flags = (runs.back().flags & ~strip) | add;
  }
  return runs;
}
int preset_of_stream(const af_engine *e, int64_t s) { return e->group_preset.empty() ? 0 : e->group_preset[s / 64]; }

// the loudness-meter rows preset k's streams own (0 without auto-makeup)
int preset_meter_slots(af_engine *e, int k) {
  const af::ChainProto &p = e->presets[k].proto;
  return (p.compressor_enabled && p.compressor.auto_makeup_enabled) ? e->presets[k].params.comp.meter_slots : 0;
}

// The height of the two state planes: the tallest preset's rows, and with live control 3 x 5 more f64 rows for each stream's
// pending dynamic-EQ coefficients (af_device.h, dyn_pending_row) behind every row a kernel addresses by itself (*first_live,
// else 0).  Reads the parameter blocks export_params wrote.
void plane_heights(af_engine *e, int *n64_out, int *n32_out, int *first_live) {
  const int n_presets = e->n_presets();
  int n64 = 0, n32 = 0;
  for (int k = 0; k < n_presets; ++k) {
    n64 = std::max(n64, af::f64_field_count(e->presets[k].params.n_eq_sections, preset_meter_slots(e, k)));
    n32 = std::max(n32, af::f32_field_count(e->presets[k].proto.limiter.lookahead_samples));
  }
  *first_live = 0;
  if (e->live_control) {
    *first_live = n64;
    n64 += 15;
  }
  *n64_out = n64;
  *n32_out = n32;
}

// The column a stream of preset k starts from: its prototype's values in the rows that do not start at zero.  `v64` / `v32`
// hold at least kF64Fixed / kF32Fixed zeros.  (upload_initial_state for every stream, af_engine_restart_streams for some.)
void initial_rows(af_engine *e, int k, double *v64, float *v32) {
  const af::CompressorProto &c = e->presets[k].proto.compressor;
  v64[af::kCompPeakEnvDb] = -120.0;
  v64[af::kCompGr] = c.current_gain_reduction_db;
  v64[af::kCompFastEnv] = c.fast_release_env_db;
  v64[af::kCompSlowEnv] = c.slow_release_env_db;
  v64[af::kCompCurReleaseMs] = c.current_release_ms;
  v64[af::kCompTargetReleaseMs] = c.target_release_ms;
  // compressor.rs:760-761: release_coeff is tc(current_release_ms) from the first sample on
  v64[af::kCompReleaseCoeff] = af::time_constant_to_coeff(c.current_release_ms, c.sample_rate);
  v64[af::kCompSmoothedMakeup] = c.smoothed_makeup_gain;
  v64[af::kCompCurrentLufs] = -100.0;
  v64[af::kLimGain] = 1.0;
  for (int i = 0; i < 3; ++i) {  // the dynamic EQ's coefficients are per-stream state (deesser.rs:536-538)
    const af::BiquadCoef &bc = e->presets[k].params.deesser.bands[i].dynamic_eq.active;
    double *d = &v64[af::kDeBand0 + i * af::kDeBandStride + 6];
    d[0] = bc.b0; d[1] = bc.b1; d[2] = bc.b2; d[3] = bc.a1; d[4] = bc.a2;
  }
  v32[af::kTpGain] = 1.0f;
}

// ... and the initial per-stream state planes.
int upload_initial_state(af_engine *e) {
  const int64_t B = e->n_streams;
  const int n_presets = e->n_presets();
  int n64 = 0, n32 = 0;
  plane_heights(e, &n64, &n32, &e->dyn_pending_row);
  if (n64 != e->n_f64 || n32 != e->n_f32) {
    e->d_st64.release();
    e->d_st32.release();
  }
  AF_HIP(e->d_st64.reserve_exact(sizeof(double) * n64 * B));
  AF_HIP(e->d_st32.reserve_exact(sizeof(float) * n32 * B));
  e->n_f64 = n64;
  e->n_f32 = n32;
  // every stream starts from its preset's prototype
  std::vector<std::vector<double>> v64s(n_presets, std::vector<double>(n64, 0.0));
  std::vector<std::vector<float>> v32s(n_presets, std::vector<float>(n32, 0.0f));
  for (int k = 0; k < n_presets; ++k) initial_rows(e, k, v64s[k].data(), v32s[k].data());
  std::vector<double> plane64((size_t)n64 * B);
  std::vector<float> plane32((size_t)n32 * B);
  for (int64_t st = 0; st < B; ++st) {
    const int k = preset_of_stream(e, st);
    for (int f = 0; f < n64; ++f) plane64[(size_t)f * B + st] = v64s[k][f];
    for (int f = 0; f < n32; ++f) plane32[(size_t)f * B + st] = v32s[k][f];
  }
  AF_HIP(hipMemcpy(e->d_st64, plane64.data(), plane64.size() * sizeof(double), hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(e->d_st32, plane32.data(), plane32.size() * sizeof(float), hipMemcpyHostToDevice));
  return AF_OK;
}

int ensure_started(af_engine *e) {
  if (!e->started && e->life.enabled && e->kernel == AF_KERNEL_STAGED)  // (refused before the device is touched)
    return fail(AF_ERR_UNSUPPORTED, "the stage pipeline keeps the streams' histories in its hand-over rings, which the per-stream "
                                    "lifecycle cannot restart, export or import: AF_KERNEL_STAGED with af_engine_set_stream_lifecycle on");
  AF_HIP(e->use_device());
  if (!e->started) {
    export_params(e);
    // the limiter's delay ring and suffix maxima live in LDS: kernel 3 (16 streams per workgroup) holds ~1000 samples
    // of lookahead (2 ms at 384 kHz = 768), kernels 1 and 2 (64 streams) ~127 / ~180
    if (e->base().proto.limiter_enabled &&
        af::quad_kernel_dynamic_lds(e->base().params.n_eq_sections, e->base().proto.limiter.lookahead_samples, true) > af::kMaxLdsBytes)
      return fail(AF_ERR_UNSUPPORTED, "limiter lookahead of %d samples exceeds what the LDS-resident ring holds",
                  e->base().proto.limiter.lookahead_samples);
    if (e->base().proto.compressor_enabled && e->base().proto.compressor.auto_makeup_enabled) {
      if (e->base().params.comp.meter_slots <= 0)
        return fail(AF_ERR_UNSUPPORTED, "auto-makeup needs a control block that divides the 400 ms loudness window "
                                        "(e.g. 480 or 960 samples at 48 kHz) and a sample rate the meter supports");
      if (e->base().params.control_block < 64)
        return fail(AF_ERR_UNSUPPORTED, "auto-makeup needs control blocks of at least 64 samples");
    }
    if (e->n_presets() > 1) {
      // several presets in one engine: the plain one-launch form of the token-ring kernel serves them (the workgroup of a
      // 64-stream group reads its own parameter block); what shapes the launch itself must agree across presets
      for (const af_preset &ps : e->presets) {
        if (ps.params.control_block != e->base().params.control_block)
          return fail(AF_ERR_INVALID_ARGUMENT, "every preset of an engine must use the same control block");
        if (ps.proto.sample_rate != e->base().proto.sample_rate) return fail(AF_ERR_INVALID_ARGUMENT, "presets must share the sample rate");
      }
      if (e->kernel != AF_KERNEL_AUTO && e->kernel != AF_KERNEL_PHASED && e->kernel != AF_KERNEL_STAGED)
        return fail(AF_ERR_UNSUPPORTED, "multi-preset engines run the token-ring kernel or the stage pipeline");
      const size_t n_groups = (size_t)(e->n_streams + 63) / 64;
      if (e->group_preset.size() != n_groups) e->group_preset.assign(n_groups, 0);
      e->d_group_preset.release();
      AF_HIP(e->d_group_preset.reserve_exact(sizeof(int32_t) * n_groups));
      AF_HIP(hipMemcpy(e->d_group_preset, e->group_preset.data(), sizeof(int32_t) * n_groups, hipMemcpyHostToDevice));
    }
    AF_HIP(e->d_params.reserve(e->presets.size()));
    AF_HIP(e->d_params_pre.reserve(1));
    AF_HIP(e->d_params_de.reserve(1));
    AF_HIP(e->d_params_eq.reserve(e->presets.size() * kEqParamSlots));  // one set of blocks per window in flight
    if (!e->d_status) {
      AF_HIP(e->d_status.reserve_exact(sizeof(int32_t) * af::kStatusWords));  // (LaunchArgs::status)
      AF_HIP(e->d_status.keep_if(hipMemset(e->d_status, 0, sizeof(int32_t) * af::kStatusWords)));
    }
    int rc = upload_initial_state(e);
    if (rc) return rc;
    if (e->supp.enabled) {
      if (e->base().proto.sample_rate != 48000.0)
        return fail(AF_ERR_INVALID_ARGUMENT, "the RNNoise suppressor runs at 48 kHz only (rnnoise.rs:3,46)");
      AF_HIP(e->supp.reset_state(e->n_streams));
    }
    e->params_dirty = true;
    e->started = true;
    e->samples_processed = 0;
    e->pending = 0;
    e->life.clear();
  }
  return AF_OK;
}

int check_device_status(af_engine *e) {
  if (!e->d_status) return AF_OK;
  int32_t st = 0;
  AF_HIP(hipMemcpy(&st, e->d_status, sizeof st, hipMemcpyDeviceToHost));
  if (st != 0)
    return fail(AF_ERR_BACKEND, "a chain kernel abandoned a stage token (device status %d); results are invalid.  (A one-launch call "
                                "waits for kernels on other streams: if something serialises dispatches, set AF_CHAIN_PERSISTENT=0.)", st);
  return AF_OK;
}

// after a launch of n samples: advance the (stream-uniform) crossfade counters
void advance_crossfades(af_engine *e, int64_t n) {
 for (af_preset &ps : e->presets) {
  af::ChainParams &o = ps.params;
  std::vector<af::SectionParams *> sections;
  for (int k = 0; k < o.n_eq_sections; ++k) sections.push_back(&o.eq[k]);
  if (o.flags & af::kFlagDeesser)
    for (auto &b : o.deesser.bands) {
      sections.push_back(&b.detector_hp);
      sections.push_back(&b.detector_lp);
      sections.push_back(&b.dynamic_eq);
    }
  for (af::SectionParams *spp : sections) {
    af::SectionParams &sp = *spp;
    if (sp.xf_remaining > 0) {
      if (n >= sp.xf_remaining) {  // promote_pending_coefficients, biquad.rs:276-286
        sp.active = sp.pending;
        sp.xf_remaining = 0;
        sp.xf_total = 0;
      } else {
        sp.xf_remaining -= (int)n;
      }
      e->params_dirty = true;
    }
  }
 }
}

// ---- live control ---------------------------------------------------------------------------------------------------
// Which mode a LIVE setter runs in: configuration (as require_config), live, or refused exactly as before the switch existed.
int setter_mode(af_engine *e, bool *live) {
  *live = false;
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (e->started) {
    if (!e->live_control) return fail(AF_ERR_STATE, "setter called after streaming started; call af_engine_reset first");
    *live = true;
    return AF_OK;
  }
  e->params_dirty = true;
  return AF_OK;
}

// The prototype of the selected preset takes over what moved on the device side since the start: the sections' active /
// pending coefficients and crossfade counters (advance_crossfades keeps them in the parameter block).  A reference setter
// applied to it afterwards then acts on the running filter: schedule() keeps `active` and restarts the counter.
void live_sync_proto(af_engine *e) {
  const int k = e->current_preset;
  e->live_retuned.resize(e->presets.size(), 0);
  e->live_retuned[(size_t)k] = 1;
  af::ChainProto &p = e->selected().proto;
  const af::ChainParams &o = e->selected().params;
  auto take = [](af::BiquadProto &b, const af::SectionParams &sp) {
    b.active = sp.active;
    b.pending = sp.pending;
    b.xf_total = sp.xf_total;
    b.xf_remaining = sp.xf_remaining;
  };
  int n = 0;
  for (int b = 0; b < af::kNumBands; ++b)
    for (int sct = 0; sct < p.eq.bands[b].processing_sections; ++sct) take(p.eq.bands[b].sections[sct], o.eq[n++]);
  for (int i = 0; i < 3; ++i) {
    take(p.deesser.bands[i].detector_hp, o.deesser.bands[i].detector_hp);
    take(p.deesser.bands[i].detector_lp, o.deesser.bands[i].detector_lp);
    take(p.deesser.bands[i].dynamic_eq, o.deesser.bands[i].dynamic_eq);
  }
}

// Record one state edit for the selected preset.  An earlier edit of the same row that nothing read since is superseded, so
// the list stays as short as the set of rows the setters touch however often they are called between two calls.
void live_op(af_engine *e, int32_t kind, int dst, int src, double value, double value2 = 0.0) {
  const int32_t preset = e->current_preset;
  auto &ops = e->retune_ops;
  for (size_t i = ops.size(); i-- > 0;) {
    if (ops[i].preset != preset) continue;
    if (ops[i].kind != af::kRetuneSet && ops[i].src == dst) break;  // read since: everything before it stays
    if (ops[i].dst == dst) {
      ops.erase(ops.begin() + (std::ptrdiff_t)i);
      break;
    }
  }
  ops.push_back(af::RetuneOp{kind, preset, dst, kind == af::kRetuneSet ? 0 : src, value, value2});
}
void live_set(af_engine *e, int row, double v) { live_op(e, af::kRetuneSet, row, 0, v); }
void live_copy(af_engine *e, int dst, int src) { live_op(e, af::kRetuneCopy, dst, src, 0.0); }
// Biquad::schedule_coefficients_crossfade, biquad.rs:256-257: the pending path starts from the live memories (rows z1 z2 pz1 pz2)
void live_restart_section(af_engine *e, int z_row) {
  live_copy(e, z_row + 2, z_row);
  live_copy(e, z_row + 3, z_row + 1);
}
// Compressor::reset_adaptive_release_state, compressor.rs:288-291
void live_reset_release_envelopes(af_engine *e) {
  live_copy(e, af::kCompFastEnv, af::kCompGr);
  live_set(e, af::kCompSlowEnv, 0.0);
}
// current_release_ms / target_release_ms / release_coeff as a setter leaves them with adaptive release off (compressor.rs:238-242)
void live_set_release(af_engine *e, const af::CompressorProto &c) {
  live_set(e, af::kCompCurReleaseMs, c.current_release_ms);
  live_set(e, af::kCompTargetReleaseMs, c.target_release_ms);
  live_set(e, af::kCompReleaseCoeff, c.release_coeff);
}

// the selected preset's parameter block follows its prototype (the next call uploads it if it changed)
int live_commit(af_engine *e) {
  af::ChainParams &o = e->selected().params;
  const int n_before = o.n_eq_sections;
  export_params(e, e->selected().proto, o);
  if ((size_t)e->current_preset < e->live_cuts.size() && e->live_cuts[(size_t)e->current_preset]) o.deesser.dyn_pending_row = e->dyn_pending_row;
  if (o.n_eq_sections != n_before) return fail(AF_ERR_BACKEND, "internal: a live setter changed the EQ's section count");
  return AF_OK;
}

// A live change of one EQ band (eq.rs:279-298 on the running band): checked first, then the prototype, the parameter block
// and the edit list.  `c` is the band's whole new configuration.
int live_eq_set_band(af_engine *e, int band, const af::EqBandConfig &c) {
  if (c.filter_type < 0 || c.filter_type > 5)
    return fail(AF_ERR_INVALID_ARGUMENT, "band %d has unsupported EQ filter type id: %d", band, c.filter_type);
  const std::string msg = af::eq_validate(c, band, e->selected().proto.sample_rate);
  if (!msg.empty()) return fail(AF_ERR_INVALID_ARGUMENT, "%s", msg.c_str());
  const af::EqProto &eq = e->selected().proto.eq;
  if (af::EqBandProto::required_sections(c) > eq.bands[band].processing_sections)
    return fail(AF_ERR_UNSUPPORTED, "band %d would need %d biquad sections and holds %d: the per-stream state planes are sized when "
                                    "streaming starts; call af_engine_reset first",
                band, af::EqBandProto::required_sections(c), eq.bands[band].processing_sections);
  live_sync_proto(e);
  int first = 0;
  for (int b = 0; b < band; ++b) first += eq.bands[b].processing_sections;
  e->selected().proto.eq.set_band_config(band, c);
  for (int sct = 0; sct < eq.bands[band].processing_sections; ++sct) live_restart_section(e, af::kEqBase + 4 * (first + sct));
  return live_commit(e);
}

// The edits recorded since the last call, in one launch on the call's stream: behind the previous call's work, ahead of this
// call's first parameter upload and kernel.  Nothing pending: nothing launched.
int launch_pending_retune(af_engine *e, hipStream_t stream) {
  e->retune_span.clear();
  if (e->retune_ops.empty()) return AF_OK;
  const size_t bytes = e->retune_ops.size() * sizeof(af::RetuneOp);
  const size_t blocks = (bytes + sizeof(af::ChainParams) - 1) / sizeof(af::ChainParams);
  AF_HIP(e->d_retune.reserve_retiring(blocks * sizeof(af::ChainParams), e->retired, stream));
  std::vector<af::ChainParams> carrier(blocks);  // (the pinned stager moves parameter blocks: the list rides in as many as it fills)
  std::memcpy(carrier.data(), e->retune_ops.data(), bytes);
  AF_HIP(e->stager.upload(e->d_retune, carrier.data(), blocks * sizeof(af::ChainParams), stream));
  af::RetuneArgs ra{};
  ra.ops = reinterpret_cast<const af::RetuneOp *>(e->d_retune.get());
  ra.group_preset = e->n_presets() == 1 ? nullptr : e->d_group_preset;
  ra.st64 = e->d_st64;
  ra.n_ops = (int32_t)e->retune_ops.size();
  ra.n_streams = e->n_streams;
  ra.n_fields = e->n_f64;
  if (e->timing) AF_HIP(e->retune_span.begin(stream));
  AF_HIP(af::launch_retune_state(ra, stream));
  if (e->timing) AF_HIP(e->retune_span.end(stream));
  e->last_launches += 1;
  e->retune_ops.clear();
  return AF_OK;
}

// The gate's parameters and state pointer on a pre-pass launch (gate.rs:158-225 for the derived constants).
void gate_args(const af_engine *e, af::SuppArgs &sa) {
  const double fs = e->sample_rate;
  sa.gate = 1;
  sa.gate_state = e->d_gate;
  sa.gate_thr = e->gate_threshold_db;
  sa.gate_rms_c = af::time_constant_to_coeff(8.0, fs);
  sa.gate_rms_omc = 1.0 - sa.gate_rms_c;
  sa.gate_atk = af::time_constant_to_coeff(e->gate_attack_ms, fs);
  sa.gate_atk_omc = 1.0 - sa.gate_atk;
  sa.gate_rel = af::time_constant_to_coeff(e->gate_release_ms, fs);
  sa.gate_rel_omc = 1.0 - sa.gate_rel;
  sa.gate_hold = (int32_t)std::round(fs * 50.0 / 1000.0);
  sa.gate_window = (int32_t)std::round(fs * 500.0 / 1000.0);
  sa.gate_cooldown = (int32_t)std::round(fs * 1000.0 / 1000.0);
  sa.gate_relax = (int32_t)std::round(fs * 700.0 / 1000.0);
  sa.gate_vad_mode = e->gate_mode != 0 ? 1 : 0;
}

void drop_vad_evidence(af_engine *e) {
  e->vad_ev_blocks = 0;
  e->vad_ev_prob.clear();
  e->vad_ev_avail.clear();
}
bool gate_vad_fused(const af_engine *e) { return e->gate_enabled && e->gate_vad_attached && e->gate_mode != 0; }

// What the fused passes read beside gate_args (every f32 evaluated as the reference evaluates it, in f32)
void vad_gate_args(const af_engine *e, af::VadGateArgs &va) {
  const double fs = e->sample_rate;
  const float fs32 = (float)(uint32_t)fs;  // VadAutoGate::sample_rate is a u32
  va.plane = e->d_gate_vad;
  va.dec = e->d_vad_dec;
  va.block = e->base().params.control_block;
  va.mode = e->gate_mode;
  va.auto_threshold = e->vad_auto_threshold ? 1 : 0;
  va.vad_threshold = e->vad_threshold;
  va.margin_db = e->vad_margin_db;
  va.manual_threshold_db = (float)e->gate_threshold_db;  // set_manual_threshold, vad.rs:996-999 (already inside [-80, -10])
  va.hold_samples = e->vad_hold_ms / 1000.0f * fs32;      // vad.rs:940
  va.debounce_samples = 50.0f / 1000.0f * fs32;           // vad.rs:929
  va.smooth_c = af::time_constant_to_coeff(35.0, fs);     // gate.rs:217-220
  va.smooth_omc = 1.0 - va.smooth_c;
  auto clampf32 = [](float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); };
  va.open_thr = clampf32(e->vad_threshold, 0.05f, 0.95f);                                // gate.rs:392
  va.close_norm = clampf32(va.open_thr - 0.12f, 0.02f, va.open_thr);                     // gate.rs:393
  va.close_relax = clampf32(va.open_thr - 0.20f, 0.02f, va.open_thr);
  va.conf_close = clampf32(va.open_thr - 0.20f, 0.02f, std::max(va.open_thr - 0.02f, 0.02f));  // gate.rs:489-490
  va.conf_span = std::max(va.open_thr - va.conf_close, 1.0e-3f);                          // gate.rs:491
  va.tail_thr = e->vad_threshold - 0.20f;                                                // gate.rs:517
}

// Before a fused call's first pass, on the caller's stream: the state plane (allocated / re-initialised when due), room for
// the call's decision rows, and the pending evidence through a pinned slot.  Fills `va` but for block0.
int vad_gate_prepare(af_engine *e, int64_t blocks, hipStream_t stream, af::VadGateArgs &va) {
  const int64_t NS = e->n_streams;
  if (!e->d_gate_vad) {
    AF_HIP(e->d_gate_vad.reserve_exact(sizeof(uint32_t) * af::kVadFields * NS));
    e->vad_ctl_fresh = e->vad_fused_fresh = true;
  }
  if (e->vad_ctl_fresh || e->vad_fused_fresh) {
    AF_HIP(af::launch_vad_plane_init(e->d_gate_vad, e->n_streams, (float)(uint32_t)e->sample_rate * 0.05f, e->vad_ctl_fresh,
                                     e->vad_fused_fresh, stream));
    e->vad_ctl_fresh = e->vad_fused_fresh = false;
  }
  AF_HIP(e->d_vad_dec.reserve_retiring((size_t)(blocks * af::kVadDecWords * NS) * sizeof(uint32_t), e->retired, stream));
  vad_gate_args(e, va);
  va.prob = nullptr;
  va.avail = nullptr;
  va.ev_stride = 0;
  if (e->vad_ev_blocks > 0) {
    const size_t count = e->vad_ev_prob.size(), bytes = count * (sizeof(float) + 1);
    AF_HIP(e->d_vad_ev.reserve_retiring(bytes, e->retired, stream));
    AF_HIP(e->ev_stager.upload(e->d_vad_ev, e->vad_ev_prob.data(), count * sizeof(float), e->vad_ev_avail.data(), count, stream));
    va.prob = reinterpret_cast<const float *>(e->d_vad_ev.get());
    va.avail = e->d_vad_ev + count * sizeof(float);
    va.ev_stride = e->vad_ev_per_stream ? NS : 0;
    e->vad_ev_blocks = 0;  // consumed: evidence is for ONE call
    e->vad_ev_prob.clear();
    e->vad_ev_avail.clear();
  }
  va.dec = e->d_vad_dec;
  e->vad_dec_blocks = blocks;
  return AF_OK;
}

// Without the suppressor, the front end runs in the gated pre-pass when the gate is on -- and for the whole stream when the
// chain's form was chosen with the front end stripped: the stage pipeline does not build the DC block / high-pass, and the
// choice holds until a reset, while the gate can be switched off between calls.
bool front_end_in_gate_prepass(const af_engine *e) {
  if (e->supp.enabled) return false;
  return e->gate_enabled || (e->pipe.active && (e->base().params.flags & (af::kFlagDcBlock | af::kFlagPreHighpass)));
}

// What the chain launches of a segment share: the engine's planes and parameter blocks (an array beside the group -> preset
// table exactly when there are several presets) and the segment.  A launch site sets only what its launch differs in.
af::LaunchArgs segment_args(const af_engine *e, const float *in, float *out, af::BlockStats *stats, int64_t n_samples,
                            int64_t stream_stride, int64_t samples_before, int32_t layout) {
  af::LaunchArgs a{};
  a.params = e->d_params;
  a.group_preset = e->n_presets() > 1 ? e->d_group_preset.get() : nullptr;
  a.st64 = e->d_st64;
  a.st32 = e->d_st32;
  a.in = in;
  a.out = out;
  a.stats = stats;
  a.status = e->d_status;
  a.n_samples = n_samples;
  a.stream_stride = stream_stride;
  a.samples_before = samples_before;
  a.n_streams = e->n_streams;
  a.layout = layout;
  return a;
}

// Several presets in one engine: one launch of the token-ring kernel, the workgroup of every 64-stream group reading its
// own parameter block.  `strip` = flags the caller's pipeline has already taken care of (the suppressor's front end).
int launch_chain_multi(af_engine *e, uint32_t strip, uint32_t add, const float *in, float *out, int64_t n_samples,
                       int64_t stream_stride, int32_t layout, int64_t samples_before, af::BlockStats *stats, hipStream_t stream,
                       bool stats_cleared) {
  for (const af_preset &ps : e->presets) {
    // (the stage pipeline runs both for several presets, when the presets agree on which stages there are: stage_pipe_serves)
    const af::ChainParams &hp = ps.params;
    if ((hp.flags & af::kFlagDeesser) || ((hp.flags & af::kFlagCompressor) && hp.comp.auto_makeup_enabled))
      return fail(AF_ERR_UNSUPPORTED, "several presets with the de-esser or auto-makeup run on the stage pipeline only, and there every "
                                      "preset must enable the same stages (de-esser ahead of the EQ, compressor, auto-makeup, limiter)");
  }
  const std::vector<af::ChainParams> runs = run_params(e, strip, add);
  size_t dyn = 0;  // every workgroup lays out its own preset: the launch needs the largest of the layouts
  for (const af::ChainParams &run : runs) {
    bool xf = false;
    for (int j = 0; j < run.n_eq_sections; ++j) xf |= run.eq[j].xf_remaining > 0;
    dyn = std::max(dyn, af::ring_kernel_dynamic_lds(run.n_eq_sections, run.lim.lookahead_samples, xf));
  }
  if (dyn > af::kMaxLdsBytes)
    return fail(AF_ERR_UNSUPPORTED, "the token-ring kernel needs more LDS than a CU has for one of the presets");
  e->last_kernel_used = AF_KERNEL_PHASED;
  const int cb = runs[0].control_block;
  const int64_t rows = ((n_samples + cb - 1) / cb) * e->n_streams;
  AF_HIP(e->d_params.sync(runs.data(), runs.size(), e->stager, stream));
  const af::LaunchArgs a = segment_args(e, in, out, stats, n_samples, stream_stride, samples_before, layout);
  af::TimedSpan span;
  if (e->timing) AF_HIP(span.begin(stream));
  if (!stats_cleared) AF_HIP(hipMemsetAsync(stats, 0, sizeof(af::BlockStats) * rows, stream));  // fields are written by their tokens
  AF_HIP(af::launch_chain_ring_lds(a, dyn, e->ring_variant, false, stream));
  e->last_launches += 1;
  if (e->timing) {
    AF_HIP(span.end(stream));
    e->chain_ms_events.push_back(std::move(span));
  }
  advance_crossfades(e, n_samples);
  return AF_OK;
}

int engine_event(af_engine *e, hipEvent_t *out_ev);

// One pass of the chain over a segment of samples for every stream: one launch, or the pre-pass + main
// pair when the compressor's auto-makeup needs whole-block input power first (compressor.rs:710).
// `params_stream` is where parameter uploads are ordered; `stream` is where the kernels run.
int launch_chain_segment(af_engine *e, const af::ChainParams &run_in, bool run_modified, const float *in, float *out,
                         int64_t n_samples, int64_t stream_stride, int32_t layout, int64_t samples_before,
                         af::BlockStats *stats, const double *vad, hipStream_t stream, hipStream_t /*caller*/,
                         bool stats_cleared = false, const double *pre_power = nullptr, const int64_t *ready = nullptr) {
  // `stats_cleared`: the rows were zeroed (and partly filled) by an earlier kernel of this window: do not clear them again
  // `pre_power`: [block][stream] compressor-input block powers of this segment, left by the systolic EQ kernel that ran as
  // the window's pre-pass: an auto-makeup segment is then ONE launch
  // `ready`: the segment is a whole call whose input arrives window by window (LaunchArgs::ready); only the plain one-launch form
  // of the token-ring kernel follows such a counter -- the caller has checked that this is what the configuration takes
  const bool followed_counter = ready != nullptr;
  if (ready && (e->n_presets() > 1 || e->kernel == AF_KERNEL_ROLES || af::switches().roles != 0))
    return fail(AF_ERR_BACKEND, "internal: only the plain token-ring launch follows a ready counter");
  if (e->n_presets() > 1)
    return launch_chain_multi(e, e->base().params.flags & ~run_in.flags, run_in.flags & af::kFlagInputDone, in, out, n_samples,
                              stream_stride, layout, samples_before, stats, stream, stats_cleared);
  af::ChainParams run = run_in;
  const int cb = run.control_block;
  const int64_t rows = ((n_samples + cb - 1) / cb) * e->n_streams;
  bool any_xf = false;
  for (int k = 0; k < run.n_eq_sections; ++k) any_xf |= run.eq[k].xf_remaining > 0;
  const bool ring_fits = af::ring_kernel_dynamic_lds(run.n_eq_sections, run.lim.lookahead_samples, any_xf) <= af::kMaxLdsBytes;
  const bool auto_makeup = (run.flags & af::kFlagCompressor) && run.comp.auto_makeup_enabled;
  const bool eq_first_deesser = (run.flags & af::kFlagDeesser) && (run.flags & af::kFlagEqBeforeDeesser);
  const bool quad_ok = !auto_makeup && !eq_first_deesser &&
                       af::quad_kernel_dynamic_lds(run.n_eq_sections, run.lim.lookahead_samples, any_xf) <= af::kMaxLdsBytes;
  int kernel = e->kernel;
  if (kernel == AF_KERNEL_AUTO || kernel == AF_KERNEL_ROLES) {
    // Kernel 2 (the token ring, 64 streams per workgroup) wherever its LDS fits: a launch lasts as long as ONE
    // workgroup needs for its streams' samples, whatever the batch, and since its waves carry priorities (in a serial
    // unit, and growing with the age of their chunk) that is shorter than kernel 3's (16 streams per workgroup, which
    // the same priorities slow down): 206-212 vs 217-225 ms for 4096 streams x 10 s of the dynamics chain, 209 vs 212 ms
    // for 256 streams.  Kernel 3 serves configurations whose limiter ring does not fit kernel 2's LDS layout.
    kernel = ring_fits ? AF_KERNEL_PHASED : (quad_ok ? AF_KERNEL_QUAD : AF_KERNEL_LANE_PER_STREAM);
  }
  if (kernel == AF_KERNEL_QUAD && !quad_ok)
    return fail(AF_ERR_UNSUPPORTED, "the quad kernel does not build auto-makeup or the EQ-before-de-esser order; use AF_KERNEL_PHASED");
  if (kernel == AF_KERNEL_PHASED && !ring_fits)
    return fail(AF_ERR_UNSUPPORTED, "the token-ring kernel needs more LDS than a CU has for this configuration");
  if (kernel == AF_KERNEL_LANE_PER_STREAM && af::lane_kernel_dynamic_lds(run.lim.lookahead_samples) > 90 * 1024)
    return fail(AF_ERR_UNSUPPORTED, "the lane-per-stream kernel cannot hold a limiter lookahead of %d samples in LDS",
                run.lim.lookahead_samples);
  if (auto_makeup && kernel != AF_KERNEL_PHASED)
    return fail(AF_ERR_UNSUPPORTED, "compressor auto-makeup is only built into the token-ring kernel");
  e->last_kernel_used = kernel;
  const bool deesser = (run.flags & af::kFlagDeesser) != 0;
  const bool eq_first = (run.flags & af::kFlagEqBeforeDeesser) != 0;
  const uint32_t front_flags = af::kFlagInputScrub | af::kFlagInputClamp | af::kFlagDcBlock | af::kFlagPreHighpass;
  const bool two_pass = (auto_makeup && !pre_power) || (deesser && eq_first);
  if (two_pass && kernel != AF_KERNEL_PHASED)
    return fail(AF_ERR_UNSUPPORTED, "EQ-before-de-esser order is only built around the token-ring kernel");
  // ---- the role pipeline (af_roles.hip): compressor and limiter as two kernels of dedicated serial waves + feed-forward
  // waves, LDS hand-over; the EQ and the block input statistics are the systolic EQ kernel's.  Where it serves the
  // configuration it replaces the token-ring launch (same state planes: the two can alternate mid-stream).
  {
    const int roles_env = af::switches().roles;
    const bool input_done = (run.flags & af::kFlagInputDone) != 0;
    const bool eq_pre_ok = layout == AF_LAYOUT_STREAM_MAJOR && !(run.flags & (af::kFlagDcBlock | af::kFlagPreHighpass)) &&
                           (!(run.flags & af::kFlagEq) || run.n_eq_sections <= 16);
    const bool comp_on = (run.flags & af::kFlagCompressor) != 0;
    const bool served = !two_pass && !deesser && !auto_makeup && af::lim_roles_serves(run) && (!comp_on || af::comp_roles_serves(run)) &&
                        (input_done || eq_pre_ok);
    if (served && (e->kernel == AF_KERNEL_ROLES || (e->kernel == AF_KERNEL_AUTO && roles_env != 0))) {
      // the limiter half on a stream of its own (the suppressor pipeline's: other CUs, a window behind the compressor)
      const hipStream_t lim_stream = (e->lim_stream && stream == e->aux_stream) ? e->lim_stream : stream;
      e->last_kernel_used = AF_KERNEL_ROLES;
      // AF_ROLES=2: the compressor stays on the token-ring kernel, which then ends at the compressor's output
      const bool ring_comp = comp_on && roles_env == 2 && ring_fits;
      af::ChainParams up = run;
      if (ring_comp) up.flags = (up.flags & ~af::kFlagLimiter) | af::kFlagCompOnly;
      AF_HIP(e->d_params.sync(&up, 1, e->stager, stream));
      af::TimedSpan span;
      if (e->timing) AF_HIP(span.begin(stream));
      if (!stats_cleared) AF_HIP(hipMemsetAsync(stats, 0, sizeof(af::BlockStats) * rows, stream));
      af::LaunchArgs ra = segment_args(e, in, out, stats, n_samples, stream_stride, samples_before, layout);
      if (!input_done) {  // EQ (or a plain pass when it is off) + block input statistics
        AF_HIP(af::launch_eq_systolic(e->d_params, nullptr, e->d_st64, in, out, nullptr, nullptr, 0, 0, stats, any_xf, n_samples,
                                      stream_stride, e->n_streams, stream));
        ra.in = out;
        e->last_launches += 1;
      }
      if (ring_comp) {
        af::ChainParams shape = up;
        shape.flags = (shape.flags & ~af::kFlagEq) | af::kFlagInputDone;  // (the systolic EQ kernel above did both)
        AF_HIP(e->d_params.sync(&shape, 1, e->stager, stream));  // (behind the EQ launch, which read `up`)
        AF_HIP(af::launch_chain_ring(ra, shape.n_eq_sections, shape.lim.lookahead_samples, any_xf, e->ring_variant, false, stream));
        ra.in = out;
        e->last_launches += 1;
      } else if (comp_on) {
        AF_HIP(af::launch_chain_comp_roles(ra, run.comp.sidechain_highpass_enabled != 0, run.comp.adaptive_release != 0, stream));
        ra.in = out;
        e->last_launches += 1;
      }
      if (e->timing) {  // (with the limiter on its own stream the bracket holds what the chain stream did)
        AF_HIP(span.end(stream));
        e->chain_ms_events.push_back(std::move(span));
      }
      if (lim_stream != stream) {
        hipEvent_t comp_done;
        if (int rc = engine_event(e, &comp_done)) return rc;
        AF_HIP(hipEventRecord(comp_done, stream));
        AF_HIP(hipStreamWaitEvent(lim_stream, comp_done, 0));
      }
      AF_HIP(af::launch_chain_lim_roles(ra, run.lim.lookahead_samples, lim_stream));
      e->last_launches += 1;
      advance_crossfades(e, n_samples);
      return AF_OK;
    }
    if (e->kernel == AF_KERNEL_ROLES) kernel = ring_fits ? AF_KERNEL_PHASED : (quad_ok ? AF_KERNEL_QUAD : AF_KERNEL_LANE_PER_STREAM);  // not served: as AUTO
  }
  af::LaunchArgs a = segment_args(e, in, out, stats, n_samples, stream_stride, samples_before, layout);
  af::TimedSpan span;
  if (e->timing) AF_HIP(span.begin(stream));
  if (two_pass || deesser) {  // (per-call scratch: the old rows are retired, not freed)
    AF_HIP(e->d_stats_pre.reserve_retiring(sizeof(af::BlockStats) * rows, e->retired, stream));
    AF_HIP(e->d_stats_de.reserve_retiring(sizeof(af::BlockStats) * rows, e->retired, stream));
  }
  const af::BlockStats *input_rows = nullptr;  // where the block input statistics end up when a side pass saw the input
  if (deesser) {
    // the de-esser pass reads the unmodified parameter block (its own copy: the chain kernels get edited flags)
    AF_HIP(e->d_params_de.sync(&run_in, 1, e->stager, stream));
    AF_HIP(hipMemsetAsync(e->d_stats_de, 0, sizeof(af::BlockStats) * rows, stream));
    if (!eq_first) {
      // routing.rs: pre-filter -> de-esser -> EQ ...: this pass takes the front end with it
      AF_HIP(af::launch_deesser(e->d_params_de, e->d_st64, e->d_st32, in, out, e->d_stats_de, n_samples, stream_stride,
                                e->n_streams, layout, true, false, stream));
      e->last_launches += 1;
      a.in = out;
      run.flags &= ~front_flags;
      input_rows = e->d_stats_de;
    }
    run.flags &= ~af::kFlagDeesser;
  }
  if (kernel == AF_KERNEL_PHASED) {
    // the ring kernel writes each stats field from the token that owns it; untouched fields must read 0
    if (!stats_cleared) AF_HIP(hipMemsetAsync(stats, 0, sizeof(af::BlockStats) * rows, stream));
    if (two_pass) {
      af::ChainParams pre = run, post = run;
      pre.flags = (pre.flags & ~(af::kFlagCompressor | af::kFlagLimiter)) | af::kFlagPrePass;
      post.flags &= ~(af::kFlagEq | front_flags);
      // both variants are uploaded only when they change (first launch; while a coefficient crossfade advances), through
      // pinned slots: no host wait inside a window loop
      AF_HIP(e->d_params_pre.sync(&pre, 1, e->stager, stream));
      AF_HIP(e->d_params.sync(&post, 1, e->stager, stream));
      AF_HIP(hipMemsetAsync(e->d_stats_pre, 0, sizeof(af::BlockStats) * rows, stream));
      af::LaunchArgs a1 = a;
      a1.params = e->d_params_pre;
      a1.stats = e->d_stats_pre;
      AF_HIP(af::launch_chain_ring(a1, pre.n_eq_sections, pre.lim.lookahead_samples, any_xf, e->ring_variant, false, stream));
      if (!input_rows) input_rows = e->d_stats_pre;
      const af::BlockStats *power_rows = e->d_stats_pre;
      if (deesser && eq_first) {
        // ... -> EQ -> de-esser -> compressor: the compressor-input block power is the de-esser's output power
        AF_HIP(af::launch_deesser(e->d_params_de, e->d_st64, e->d_st32, out, out, e->d_stats_de, n_samples, stream_stride,
                                  e->n_streams, layout, false, auto_makeup, stream));
        e->last_launches += 1;
        power_rows = e->d_stats_de;
      }
      af::LaunchArgs a2 = a;
      a2.in = out;
      if (auto_makeup) {
        a2.pre_stats = power_rows;
        a2.vad_prob = vad;
      }
      AF_HIP(af::launch_chain_ring(a2, post.n_eq_sections, post.lim.lookahead_samples, any_xf, e->ring_variant, auto_makeup, stream));
      e->last_launches += 2;
    } else {
      AF_HIP(e->d_params.sync(&run, 1, e->stager, stream));
      if (auto_makeup) {  // the systolic EQ kernel was this segment's pre-pass
        a.pre_power = pre_power;
        a.vad_prob = vad;
      }
      a.ready = ready;
      ready = nullptr;  // (taken)
      AF_HIP(af::launch_chain_ring(a, run.n_eq_sections, run.lim.lookahead_samples, any_xf, e->ring_variant, auto_makeup, stream));
      e->last_launches += 1;
    }
  } else {
    AF_HIP(e->d_params.sync(&run, 1, e->stager, stream));
    if (kernel == AF_KERNEL_QUAD) {
      AF_HIP(hipMemsetAsync(stats, 0, sizeof(af::BlockStats) * rows, stream));  // fields are written by their tokens
      AF_HIP(af::launch_chain_quad(a, run.n_eq_sections, run.lim.lookahead_samples, any_xf, e->ring_variant ? e->ring_variant / 100 : 12, stream));
    } else {
      AF_HIP(af::launch_chain_lane(a, run.lim.lookahead_samples, stream));
    }
    e->last_launches += 1;
  }
  if (ready) return fail(AF_ERR_BACKEND, "internal: a launch that follows a ready counter took a path that does not read it");
  if (input_rows || deesser) {
    AF_HIP(af::launch_merge_side_stats(stats, input_rows, deesser ? e->d_stats_de : nullptr, rows, stream));
    e->last_launches += 1;
  }
  if (e->timing) {
    AF_HIP(span.end(stream));
    e->chain_ms_events.push_back(std::move(span));
  }
  if (!followed_counter) advance_crossfades(e, n_samples);  // (a one-launch call: the caller moves the counters window by window)
  return AF_OK;
}


// an event of the engine's pool, valid until the end of the current process call
int engine_event(af_engine *e, hipEvent_t *out_ev) {
  if (e->ev_cursor == e->sync_events.size()) {
    af::Event ev;
    AF_HIP(ev.create(hipEventDisableTiming));
    e->sync_events.push_back(std::move(ev));
  }
  *out_ev = e->sync_events[e->ev_cursor++].get();
  return AF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The stage-pipeline form of the chain (af_stages.hip).  Which configurations it serves:
bool stage_pipe_serves_one(const af::ChainParams &run) {
  if (run.flags & (af::kFlagDcBlock | af::kFlagPreHighpass | af::kFlagPrePass)) return false;
  // the de-esser in its default place (ahead of the EQ) runs as stages of its own; EQ-before-de-esser stays on kernel 2
  if ((run.flags & af::kFlagDeesser) && (run.flags & af::kFlagEqBeforeDeesser)) return false;
  if ((run.flags & af::kFlagEq) && run.n_eq_sections > 16) return false;
  if ((run.flags & af::kFlagLimiter) && run.lim.lookahead_samples > af::kMaxLookahead) return false;
  return true;
}
// `run`: preset 0 as the chain will see it (the front end's flags stripped when the suppressor's pre-pass owns them)
bool stage_pipe_serves(af_engine *e, const af::ChainParams &run, int32_t layout) {
  if (layout != AF_LAYOUT_STREAM_MAJOR || !stage_pipe_serves_one(run)) return false;
  const uint32_t strip = e->base().params.flags & ~run.flags;
  for (int k = 1; k < e->n_presets(); ++k) {
    // several presets: every group's stages run as roles of the same dispatches, so the presets must agree on which stages
    // there are and which code paths they take (what differs freely: every coefficient, the EQ, the limiter's lookahead)
    af::ChainParams other = e->presets[k].params;
    other.flags &= ~strip;
    const uint32_t shape = af::kFlagCompressor | af::kFlagLimiter | af::kFlagDeesser;
    if (!stage_pipe_serves_one(other) || (other.flags & shape) != (run.flags & shape) ||
        other.comp.sidechain_highpass_enabled != run.comp.sidechain_highpass_enabled ||
        other.comp.adaptive_release != run.comp.adaptive_release || other.comp.auto_makeup_enabled != run.comp.auto_makeup_enabled ||
        other.control_block != run.control_block)
      return false;
  }
  return true;
}

size_t pow2_at_least(int64_t n) {
  size_t p = 1;
  while ((int64_t)p < n) p <<= 1;
  return p;
}

// rings sized for windows of up to `tw_max` samples
int stage_pipe_prepare(af_engine *e, int64_t tw_max) {
  auto &sp = e->pipe;
  {  // the per-block arrays (makeup gains, block powers): a reset may have brought a shorter control block, i.e. more blocks
    const int cb = e->base().params.control_block;
    const int64_t rows = ((std::max(tw_max, sp.tw_max) + cb - 1) / cb + 1) * e->n_streams;
    if (rows > sp.mk_rows) {
      if (sp.d_mk || sp.d_bp) AF_HIP(hipDeviceSynchronize());
      sp.mk_rows = 0;
      AF_HIP(sp.d_mk.reserve_exact(sizeof(double) * rows * af_engine::StagePipe::kMkSets));
      AF_HIP(sp.d_bp.reserve_exact(sizeof(double) * rows * af_engine::StagePipe::kBpSets));
      sp.mk_rows = rows;
    }
  }
  if (sp.rings.xe && tw_max <= sp.tw_max && sp.with_deesser == ((e->base().params.flags & af::kFlagDeesser) != 0)) return AF_OK;
  if (sp.rings.xe) {  // grow: only between calls of a fresh engine (the rings hold the histories)
    if (sp.windows > 0 && tw_max > sp.tw_max)
      return fail(AF_ERR_UNSUPPORTED, "a call of %lld samples per window after smaller ones: the stage pipeline's rings were sized for %lld",
                  (long long)tw_max, (long long)sp.tw_max);
    AF_HIP(hipDeviceSynchronize());
    sp.allocs.clear();
    sp.rings = af::StageRings{};
  }
  const int64_t groups = (e->n_streams + 63) / 64;
  const int64_t hist = 2 * (af::kMaxLookahead + 1) + 64;
  // a ring holds the windows between its producer and its last consumer, one more, and the history: the stages advance in lock
  // step, an f64 ring's reader two windows behind its writer at most, the EQ output's last reader seven
  const bool deesser = (e->base().params.flags & af::kFlagDeesser) != 0;
  // (with the de-esser: a band's coefficients wait three launch steps for the third dynamic EQ of the cascade, and the chain
  // input nine for nothing -- the EQ now reads the de-esser's output ring)
  const size_t r64 = pow2_at_least((deesser ? 6 : 4) * tw_max + hist), r32 = pow2_at_least(10 * tw_max + hist);
  sp.rings.rows_f64 = (int32_t)r64;
  sp.rings.rows_f32 = (int32_t)r32;
  auto ring = [&](void **p, size_t bytes) -> hipError_t {
    af::DeviceBuffer<> buf;
    if (hipError_t err = buf.reserve_exact(bytes); err != hipSuccess) return err;
    *p = buf.get();
    sp.allocs.push_back(std::move(buf));
    return hipMemset(*p, 0, bytes);
  };
  auto ring32 = [&](float **p) { return ring(reinterpret_cast<void **>(p), sizeof(float) * r32 * 64 * groups); };
  auto ring64 = [&](double **p) { return ring(reinterpret_cast<void **>(p), sizeof(double) * r64 * 64 * groups); };
  af::StageRings &r = sp.rings;
  for (float **p : {&r.xi, &r.xe, &r.xc, &r.sfx, &r.xl, &r.itp, &r.tgt, &r.gt, &r.od}) AF_HIP(ring32(p));
  for (double **p : {&r.d, &r.pr, &r.low_e, &r.voiced_e, &r.pres_e, &r.rms_e, &r.ipk_db, &r.rms_db, &r.w_db, &r.peak_db, &r.target, &r.gr, &r.glin, &r.fast_r, &r.slow_r, &r.tgt_ms, &r.tg, &r.g})
    AF_HIP(ring64(p));
  if (deesser) {
    for (int b = 0; b < 3; ++b) {
      for (double **p : {&r.de_env[b], &r.de_ct[b], &r.de_ratio[b], &r.de_aux[b], &r.de_tr[b], &r.de_gdb[b], &r.de_red[b]}) AF_HIP(ring64(p));
      AF_HIP(ring32(&r.de_upd[b]));
      for (int j = 0; j < 5; ++j) AF_HIP(ring64(&r.de_c[b][j]));
      AF_HIP(ring32(&r.de_y[b]));
    }
    AF_HIP(ring64(&r.de_bb));
  }
  sp.with_deesser = deesser;
  sp.tw_max = tw_max;
  if (!sp.stream) {  // (a queue of its own: a CU-masked stream with every CU enabled; plain streams share a few hardware queues)
    hipDeviceProp_t prop;
    AF_HIP(hipGetDeviceProperties(&prop, e->device));
    std::vector<uint32_t> mask((size_t)(prop.multiProcessorCount + 31) / 32, 0u);
    for (int bit = 0; bit < prop.multiProcessorCount; ++bit) mask[bit >> 5] |= 1u << (bit & 31);
    if (sp.stream.create_with_cu_mask((uint32_t)mask.size(), mask.data()) != hipSuccess) {
      (void)hipGetLastError();
      AF_HIP(sp.stream.create());
    }
  }
  return AF_OK;
}

int stage_pipe_clear(af_engine *e) {  // a fresh engine: the histories are zeros
  auto &sp = e->pipe;
  if (!sp.rings.xe) return AF_OK;
  const int64_t groups = (e->n_streams + 63) / 64;
  af::StageRings &r = sp.rings;
  for (float *p : {r.xi, r.xe, r.xc, r.sfx, r.xl, r.itp, r.tgt, r.gt, r.od}) AF_HIP(hipMemset(p, 0, sizeof(float) * r.rows_f32 * 64 * groups));
  for (double *p : {r.d, r.pr, r.low_e, r.voiced_e, r.pres_e, r.rms_e, r.ipk_db, r.rms_db, r.w_db, r.peak_db, r.target, r.gr, r.glin, r.fast_r, r.slow_r, r.tgt_ms, r.tg, r.g})
    AF_HIP(hipMemset(p, 0, sizeof(double) * r.rows_f64 * 64 * groups));
  if (sp.with_deesser) {
    for (int b = 0; b < 3; ++b) {
      for (double *p : {r.de_env[b], r.de_ct[b], r.de_ratio[b], r.de_aux[b], r.de_tr[b], r.de_gdb[b], r.de_red[b]}) AF_HIP(hipMemset(p, 0, sizeof(double) * r.rows_f64 * 64 * groups));
      AF_HIP(hipMemset(r.de_upd[b], 0, sizeof(float) * r.rows_f32 * 64 * groups));
      for (int j = 0; j < 5; ++j) AF_HIP(hipMemset(r.de_c[b][j], 0, sizeof(double) * r.rows_f64 * 64 * groups));
      AF_HIP(hipMemset(r.de_y[b], 0, sizeof(float) * r.rows_f32 * 64 * groups));
    }
    AF_HIP(hipMemset(r.de_bb, 0, sizeof(double) * r.rows_f64 * 64 * groups));
  }
  sp.windows = 0;
  return AF_OK;
}

// The parameter block(s) the stage kernels read: preset 0 alone, or all presets as an array beside the group -> preset table.
int stage_chain_params(af_engine *e, hipStream_t stream) {
  auto &sp = e->pipe;
  const std::vector<af::ChainParams> runs = run_params(e, sp.strip);
  sp.w_min = 1 << 30;
  for (const af::ChainParams &run : runs) sp.w_min = std::min<int32_t>(sp.w_min, run.lim.lookahead_samples + 1);
  AF_HIP(e->d_params.sync(runs.data(), runs.size(), e->stager, stream));
  return AF_OK;
}

// ---- the pipeline as one launch per step (af_stages.h, DiagArgs): launch j runs stage k on window j - skew(k) -----------------
// The stages of this configuration in chain order, each one launch step behind the stage it reads from.
struct StagePlan {
  int stage[af::kStCount], skew[af::kStCount], n = 0;
  int depth = 0;  // the last stage's skew: launches a window needs to leave the pipeline after it entered
};
StagePlan stage_plan(const af::ChainParams &run) {
  StagePlan p;
  const bool comp = (run.flags & af::kFlagCompressor) != 0, lim = (run.flags & af::kFlagLimiter) != 0;
  auto add = [&](int k, int sk) { p.stage[p.n] = k; p.skew[p.n] = sk; ++p.n; p.depth = std::max(p.depth, sk); return sk; };
  int at = 0;
  if (run.flags & af::kFlagDeesser) {
    // the de-esser ahead of the EQ (deesser.rs:405-547): transposing loader | three detectors | levels and confidence targets |
    // three confidence / baseline recurrences | target scaling | three reduction smoothers with the gain hold | coefficients
    // (and the block's figure) | three cascaded dynamic EQs
    add(af::kStDe0, 0);
    for (int k : {af::kStDe1a, af::kStDe1b, af::kStDe1c}) add(k, 1);
    add(af::kStDe2, 2);
    for (int k : {af::kStDe3a, af::kStDe3b, af::kStDe3c}) add(k, 3);
    add(af::kStDe4s, 4);
    for (int k : {af::kStDe4a, af::kStDe4b, af::kStDe4c}) add(k, 5);
    add(af::kStDe4t, 6);
    add(af::kStDe5, 6);
    add(af::kStDe6a, 7);
    add(af::kStDe6b, 8);
    add(af::kStDe6c, 9);
    at = add(af::kStEq, 10);
  } else {
    at = add(af::kStEq, 0);
  }
  const int eq_at = at;
  add(af::kStIn, 1);  // (the xi ring: written by the EQ stage, or by the de-esser's loader, one step earlier)
  if (comp) {
    for (int k : {af::kStCompA, af::kStCompA2, af::kStF1, af::kStCompC, af::kStF2, af::kStCompE}) at = add(k, at + 1);
    if (run.comp.adaptive_release) {
      add(af::kStFR, at + 1);
      add(af::kStRel, at + 2);
    }
    if (run.comp.auto_makeup_enabled) {
      add(af::kStPow, eq_at + 1);
      at = add(af::kStF3a, at + 1);
      at = add(af::kStMakeup, at + 1);
    } else {
      at = add(af::kStF3, at + 1);
    }
  }
  if (lim)
    for (int k : {af::kStF4, af::kStLim, af::kStF5, af::kStTp}) at = add(k, at + 1);
  at = add(af::kStOut, at + 1);
  add(af::kStF6, at + 1);
  return p;
}

// launch step j of a call whose windows are `wins`: every stage whose window exists
int stage_diag_step(af_engine *e, const af::ChainParams &run, const StagePlan &plan, const std::vector<af::DiagWin> &wins, int64_t j,
                    hipStream_t stream) {
  auto &sp = e->pipe;
  af::DiagArgs d{};
  d.base.params = e->d_params;
  d.base.group_preset = e->n_presets() == 1 ? nullptr : e->d_group_preset;
  d.base.st64 = e->d_st64;
  d.base.st32 = e->d_st32;
  d.base.n_streams = e->n_streams;
  d.base.w_min = sp.w_min;
  d.base.r = sp.rings;
  d.params_eq = e->d_params_eq;
  d.flags = run.flags;
  d.sidechain = run.comp.sidechain_highpass_enabled;
  d.adaptive = run.comp.adaptive_release;
  d.auto_makeup = (run.flags & af::kFlagCompressor) && run.comp.auto_makeup_enabled;
  d.base.stream_stride = sp.call_stride;
  d.deesser = (run.flags & af::kFlagDeesser) ? 1 : 0;
  d.debug_skip = af::switches().stage_skip;  // AF_STAGE_SKIP=<StageId>: timing probe (that stage does nothing; results are garbage)
  // two dispatches per step: the one-wave workgroups (serial stages and F4), then the wide stages; with the de-esser a third
  // for its serial stages
  for (int pass = 0; pass < (d.deesser ? 3 : 2); ++pass) {
    unsigned blocks = 0;
    d.n_roles = 0;
    for (int i = 0; i < plan.n; ++i) {
      const int k = plan.stage[i];
      if (af::stage_dispatch_kind(k) != pass) continue;
      const int64_t wi = j - plan.skew[i];
      if (wi < 0 || wi >= (int64_t)wins.size()) continue;
      af::DiagRole &role = d.roles[d.n_roles++];
      role.stage = k;
      role.win = wins[(size_t)wi];
      unsigned gy = 1;
      role.gx = af::stage_role_blocks(k, role.win.n0, role.win.n, e->n_streams, d.base.w_min, &gy);
      role.first_block = blocks;
      blocks += role.gx * gy;
    }
    if (d.n_roles == 0) continue;
    const bool timed = e->timing && pass == 0;  // the serial stages' dispatch is what a step lasts: what af_engine_last_chain_launch_ms reports
    af::TimedSpan span;
    if (timed) AF_HIP(span.begin(stream));
    AF_HIP(af::launch_stage_diag(d, blocks, pass, stream));
    if (timed) {
      AF_HIP(span.end(stream));
      e->chain_ms_events.push_back(std::move(span));
    }
    e->last_launches += 1;
  }
  return AF_OK;
}

// The engine's side streams (created once).  With queue CU masks: the chain stream on as many CUs as the chain has workgroups,
// every other stream on the rest.
int ensure_side_streams(af_engine *e, hipStream_t stream) {
  if (af::switches().serial_streams) {  // AF_SERIAL_STREAMS, diagnostic: every stage on the caller's stream (per-kernel times without overlap)
    for (af::Stream *side : {&e->aux_stream, &e->pre_stream, &e->ana_stream, &e->fin_stream, &e->eq_stream}) side->borrow(stream);
  }

  if (!e->aux_stream) {
    // CU partition.  A 16-wave chain workgroup needs a whole CU (it fills the register file), and the suppressor's
    // kernels keep thousands of small, some of them long-lived, workgroups in flight: left to the dispatcher, every chain
    // launch waits for CUs to drain and runs beside strangers.  So the chain stream is confined to as many CUs as it has
    // workgroups (mask bits 0.. select the same CU indices on every XCD: tools/probe/cu_mask_probe.hip) and the
    // suppressor's streams to the rest; neither side ever waits for the other's workgroups to leave.
    int chain_cus = 0;
    const int forced_cus = af::switches().cu_partition;  // AF_CU_PARTITION: 0 no masks, N > 0 that many CUs, else automatic
    const int chain_groups = (e->n_streams + 63) / 64;
    hipDeviceProp_t prop;
    AF_HIP(hipGetDeviceProperties(&prop, e->device));
    const int total_cus = prop.multiProcessorCount;
    if (forced_cus != 0 && total_cus % 32 == 0 && total_cus <= 1024) {
      // (a power of two: the workgroups of a launch are dealt to the XCDs in turn and 48 or 56 enabled CUs leave some of them
      // with two workgroups each -- 3072 streams: 356 ms of chain launches per step on 48 CUs, 197 on 64)
      int pow2 = 8;
      while (pow2 < chain_groups) pow2 *= 2;
      chain_cus = forced_cus > 0 ? forced_cus : pow2;
      if (chain_cus * 2 > total_cus) chain_cus = 0;  // a chain that wants half the chip or more shares all of it
    }
    if (chain_cus > 0) {
      // AF_ROLES=2: the limiter half of the chain gets CUs of its own (AF_LIM_CUS, default as many as the chain), taken from
      // the suppressor's share
      int lim_cus = 0;
      if (af::switches().roles == 2) {
        lim_cus = af::switches().lim_cus >= 0 ? af::switches().lim_cus : chain_cus;
        if (lim_cus < 0 || chain_cus + lim_cus + 32 > total_cus) lim_cus = 0;
      }
      std::vector<uint32_t> chain_mask(total_cus / 32, 0u), rest_mask(total_cus / 32, 0u), lim_mask(total_cus / 32, 0u);
      // the chain takes mask bits 0.. (CU indices 0.. of every XCD), the limiter half the next ones
      for (int bit = 0; bit < total_cus; ++bit)
        (bit < chain_cus ? chain_mask : (bit < chain_cus + lim_cus ? lim_mask : rest_mask))[bit >> 5] |= 1u << (bit & 31);
      hipError_t err = e->aux_stream.create_with_cu_mask((uint32_t)chain_mask.size(), chain_mask.data());
      if (err == hipSuccess && lim_cus > 0) err = e->lim_stream.create_with_cu_mask((uint32_t)lim_mask.size(), lim_mask.data());
      for (af::Stream *rest : {&e->pre_stream, &e->ana_stream, &e->syn_stream, &e->fin_stream, &e->eq_stream})
        if (err == hipSuccess) err = rest->create_with_cu_mask((uint32_t)rest_mask.size(), rest_mask.data());
      if (err != hipSuccess) {  // platform without queue CU masks: plain streams
        (void)hipGetLastError();
        for (af::Stream *st : {&e->aux_stream, &e->pre_stream, &e->ana_stream, &e->syn_stream, &e->fin_stream, &e->eq_stream, &e->lim_stream}) st->reset();
        chain_cus = 0;
      }
    }
    e->partition_chain_cus = chain_cus;
  }
  for (af::Stream *side : {&e->aux_stream, &e->pre_stream, &e->ana_stream, &e->fin_stream, &e->eq_stream})
    if (!*side) AF_HIP(side->create());
  return AF_OK;
}

// the EQ stage's parameter block for the window about to enter the pipeline (stream-ordered behind the previous window's launch)
int stage_diag_eq_params(af_engine *e, hipStream_t stream, bool *crossfade, int32_t *slot_out) {
  std::vector<af::ChainParams> runs = run_params(e, e->pipe.strip);
  *crossfade = false;
  bool deesser = false;
  for (af::ChainParams &run : runs) {
    for (int k = 0; k < run.n_eq_sections; ++k) *crossfade |= run.eq[k].xf_remaining > 0;
    if (run.flags & af::kFlagDeesser) {
      deesser = true;
      run.flags &= ~(af::kFlagInputScrub | af::kFlagInputClamp);  // the de-esser's loader stage scrubbed the input already
    }
  }
  // With the de-esser every window keeps a parameter block of its own for as long as it is in the pipeline: the de-esser's
  // stages read their filters' crossfade counters as of the window's first sample up to eight launch steps after it entered.
  if (deesser) {
    const size_t first = (size_t)(e->eq_slot_cursor++ % kEqParamSlots) * runs.size();
    AF_HIP(e->d_params_eq.send(first, runs.data(), runs.size(), e->stager, stream));
    *slot_out = (int32_t)first;
    return AF_OK;
  }
  *slot_out = 0;
  AF_HIP(e->d_params_eq.sync(runs.data(), runs.size(), e->stager, stream));
  return AF_OK;
}

}  // namespace

extern "C" {

int af_version(void) { return 101; }
const char *af_last_error(void) { return af_last_error_text.c_str(); }

int af_device_count(void) {
  int n = 0;
  hipError_t err = hipGetDeviceCount(&n);
  if (err != hipSuccess) return fail(AF_ERR_BACKEND, "hipGetDeviceCount failed: %s", hipGetErrorString(err));
  return n;
}

int af_engine_create(double sample_rate, int32_t n_streams, int32_t device, af_engine **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (!std::isfinite(sample_rate) || sample_rate <= 0.0)
    return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be positive and finite");
  if (n_streams <= 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be positive");
  if (device < 0) return fail(AF_ERR_INVALID_ARGUMENT, "device must be >= 0");
  *out = new af_engine(sample_rate, n_streams, device);
  return AF_OK;
}

void af_engine_destroy(af_engine *e) { delete e; }

int af_engine_reset(af_engine *e) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (e->started) {
    AF_HIP(e->use_device());
    AF_HIP(hipDeviceSynchronize());
    e->retired.collect(true);
  }
  e->started = false;
  for (af::Mirrored<af::ChainParams> *m : {&e->d_params, &e->d_params_pre, &e->d_params_de, &e->d_params_eq}) m->invalidate();
  e->pipe.decided = false;
  e->params_dirty = true;
  e->samples_processed = 0;
  e->last_blocks = 0;
  e->pending = 0;
  e->last_output_samples = 0;
  e->trace_frames = 0;
  // live control: what is pending is dropped; a preset that was retuned live restarts like the reference's reset() -- every
  // filter from its configured target (Biquad::reset, biquad.rs:341-347), not from wherever a crossfade stood
  e->retune_ops.clear();
  e->retune_span.clear();
  for (size_t k = 0; k < e->live_retuned.size() && k < e->presets.size(); ++k) {
    if (!e->live_retuned[k]) continue;
    af::ChainProto &p = e->presets[k].proto;
    p.eq.reset();
    for (auto &b : p.deesser.bands) {
      b.detector_hp.reset();
      b.detector_lp.reset();
      b.dynamic_eq.reset();
    }
  }
  e->live_retuned.clear();
  e->live_cuts.clear();
  e->life.clear();  // every stream restarts with the engine (the switch is kept)
  if (e->d_gate) {  // NoiseGate::reset, gate.rs:759-785: every state field back to its initial value
    AF_HIP(e->use_device());
    AF_HIP(hipMemset(e->d_gate, 0, sizeof(int64_t) * af::kGateFields * e->n_streams));
  }
  // ... + VadAutoGate::reset (vad.rs:1017-1031): the plane is rewritten in front of the next fused pass; pending evidence is
  // dropped with vad_external_probability / _available (gate.rs:775-776)
  e->vad_ctl_fresh = e->vad_fused_fresh = true;
  e->vad_ev_blocks = 0;
  e->vad_ev_prob.clear();
  e->vad_ev_avail.clear();
  e->vad_dec_blocks = 0;
  if (e->rs_in) (void)af_stream_resampler_reset(e->rs_in);    // fresh resamplers on both sides: zero history, nothing queued
  if (e->rs_out) (void)af_stream_resampler_reset(e->rs_out);
  if (e->mix) (void)af_mixdown_reset(e->mix);  // a fresh PhaseSafeMonoState and fresh diagnostics (a new input stream)
  if (e->ow) (void)af_output_writer_reset(e->ow);  // dsp_loop.rs:796-802; the fill evidence is dropped with it
  e->ow_fill.clear();
  e->ow_fill_dirty = true;
  std::fill(e->ow_written.begin(), e->ow_written.end(), 0);
  return AF_OK;
}

int32_t af_engine_n_streams(const af_engine *e) { return e ? e->n_streams : 0; }

int af_engine_set_live_control(af_engine *e, int32_t enabled) {
  if (int rc = require_config(e)) return rc;
  e->live_control = enabled != 0;
  return AF_OK;
}
int af_engine_live_control_pending(const af_engine *e, int32_t *ops) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (ops) *ops = (int32_t)e->retune_ops.size();
  return AF_OK;
}
int af_engine_last_retune_ms(af_engine *e, double *ms) {
  if (!e || !ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  *ms = 0.0;
  if (!e->timing || !e->retune_span.used()) return AF_OK;
  AF_HIP(e->use_device());
  AF_HIP(e->retune_span.elapsed_ms(ms));
  return AF_OK;
}

#define AF_SETTER(expr)              \
  do {                               \
    int rc__ = require_config(e);    \
    if (rc__) return rc__;           \
    expr;                            \
    return AF_OK;                    \
  } while (0)

int af_engine_set_deesser_enabled(af_engine *e, int32_t on) { AF_SETTER(e->selected().proto.deesser_enabled = e->selected().proto.deesser.enabled = on != 0); }
int af_engine_set_eq_enabled(af_engine *e, int32_t on) { AF_SETTER(e->selected().proto.eq_enabled = e->selected().proto.eq.enabled = on != 0); }
int af_engine_set_compressor_enabled(af_engine *e, int32_t on) { AF_SETTER(e->selected().proto.compressor_enabled = e->selected().proto.compressor.enabled = on != 0); }
int af_engine_set_limiter_enabled(af_engine *e, int32_t on) { AF_SETTER(e->selected().proto.limiter_enabled = e->selected().proto.limiter.enabled = on != 0); }
int af_engine_set_eq_before_deesser(af_engine *e, int32_t on) { AF_SETTER(e->selected().proto.eq_before_deesser = on != 0); }
// the front end belongs to the engine, not to a preset (with the suppressor on it runs in the suppressor's pre-pass)
#define AF_ALL_PRESETS(stmt) \
  for (af_preset &ps__ : e->presets) { af::ChainProto &p = ps__.proto; stmt; }
int af_engine_set_input_scrub_enabled(af_engine *e, int32_t on) { AF_SETTER(AF_ALL_PRESETS(p.input_scrub = on != 0)); }
int af_engine_set_input_clamp_enabled(af_engine *e, int32_t on) { AF_SETTER(AF_ALL_PRESETS(p.input_clamp = on != 0)); }
int af_engine_set_prefilter_enabled(af_engine *e, int32_t on, int32_t hp) {
  AF_SETTER(AF_ALL_PRESETS((p.dc_block = on != 0, p.pre_highpass = on != 0 && hp != 0)));
}
int af_engine_set_control_block_samples(af_engine *e, int32_t n) {
  if (n < 1 || n > 8192) return fail(AF_ERR_INVALID_ARGUMENT, "control block must be in [1, 8192] samples");
  AF_SETTER(AF_ALL_PRESETS(p.control_block = n));
}

// A live setter: in configuration mode exactly AF_SETTER; after streaming started with live control on, `apply` acts on the
// prototype once it has caught up with the device (live_sync_proto), `record` lists the state edits, and the preset's
// parameter block is re-exported.  `check`: what must hold for the live form, tested before anything is touched.
#define AF_LIVE_SETTER(check, apply, record)             \
  do {                                                   \
    bool live__ = false;                                 \
    if (int rc__ = setter_mode(e, &live__)) return rc__; \
    if (live__) {                                        \
      check;                                             \
      live_sync_proto(e);                                \
    }                                                    \
    apply;                                               \
    if (live__) {                                        \
      record;                                            \
      return live_commit(e);                             \
    }                                                    \
    return AF_OK;                                        \
  } while (0)
#define AF_LIVE_PARAM_SETTER(apply) AF_LIVE_SETTER((void)0, apply, (void)0)

// the EQ's legacy setters change one field of the band's configuration (eq.rs:406-438)
#define AF_EQ_LIVE_FIELD(field, value, config_call)                      \
  do {                                                                   \
    if (int rc__ = check_band(band)) return rc__;                        \
    bool live__ = false;                                                 \
    if (int rc__ = setter_mode(e, &live__)) return rc__;                 \
    if (live__) {                                                        \
      af::EqBandConfig c__ = e->selected().proto.eq.bands[band].config;               \
      c__.field = (value);                                               \
      return live_eq_set_band(e, band, c__);                             \
    }                                                                    \
    config_call;                                                         \
    return AF_OK;                                                        \
  } while (0)
int af_eq_set_band_frequency(af_engine *e, int32_t band, double hz) { AF_EQ_LIVE_FIELD(frequency_hz, hz, e->selected().proto.eq.set_band_frequency(band, hz)); }
int af_eq_set_band_gain(af_engine *e, int32_t band, double db) { AF_EQ_LIVE_FIELD(gain_db, db, e->selected().proto.eq.set_band_gain(band, db)); }
int af_eq_set_band_q(af_engine *e, int32_t band, double q) { AF_EQ_LIVE_FIELD(q, q, e->selected().proto.eq.set_band_q(band, q)); }
int af_eq_set_band_config(af_engine *e, int32_t band, const af_eq_band_config *c) {
  if (int rc = check_band(band)) return rc;
  if (!c) return fail(AF_ERR_INVALID_ARGUMENT, "config is null");
  bool live = false;
  if (int rc = setter_mode(e, &live)) return rc;
  if (live) return live_eq_set_band(e, band, to_cfg(*c));
  e->selected().proto.eq.set_band_config(band, to_cfg(*c));
  return AF_OK;
}
int af_eq_reset(af_engine *e) { AF_SETTER(e->selected().proto.eq.reset()); }
int af_eq_band_config_validate(const af_eq_band_config *c, int32_t index, double sample_rate) {
  if (!c) return fail(AF_ERR_INVALID_ARGUMENT, "config is null");
  if (c->filter_type < 0 || c->filter_type > 5)
    return fail(AF_ERR_INVALID_ARGUMENT, "band %d has unsupported EQ filter type id: %d", index, c->filter_type);
  const std::string msg = af::eq_validate(to_cfg(*c), index, sample_rate);
  if (!msg.empty()) return fail(AF_ERR_INVALID_ARGUMENT, "%s", msg.c_str());
  return AF_OK;
}

// Live (compressor.rs:210-371 on the running compressor): what each setter edits beyond its parameters is recorded as state edits.
int af_compressor_set_threshold(af_engine *e, double v) {
  AF_LIVE_SETTER((void)0, e->selected().proto.compressor.set_threshold(v), live_reset_release_envelopes(e));
}
int af_compressor_set_ratio(af_engine *e, double v) { AF_LIVE_PARAM_SETTER(e->selected().proto.compressor.set_ratio(v)); }
int af_compressor_set_attack_time(af_engine *e, double v) { AF_LIVE_PARAM_SETTER(e->selected().proto.compressor.set_attack_time(v)); }
int af_compressor_set_release_time(af_engine *e, double v) {
  AF_LIVE_SETTER((void)0, e->selected().proto.compressor.set_release_time(v),
                 if (!e->selected().proto.compressor.adaptive_release) live_set_release(e, e->selected().proto.compressor));
}
int af_compressor_set_makeup_gain(af_engine *e, double v) {
  AF_LIVE_SETTER((void)0, e->selected().proto.compressor.set_makeup_gain(v),
                 if (!e->selected().proto.compressor.auto_makeup_enabled) live_set(e, af::kCompSmoothedMakeup, v));
}
// the stage pipeline runs every preset's stages as roles of the same dispatches: its presets take the same code paths
#define AF_LIVE_SAME_PATHS_CHECK(what)                                                                                            \
  if (e->pipe.active && e->n_presets() > 1)                                                                                       \
    return fail(AF_ERR_UNSUPPORTED, what " cannot change live on a multi-preset engine that runs the stage pipeline: every preset " \
                                         "must take the same code paths; call af_engine_reset first")
int af_compressor_set_adaptive_release(af_engine *e, int32_t on) {
  AF_LIVE_SETTER(AF_LIVE_SAME_PATHS_CHECK("adaptive release"), e->selected().proto.compressor.set_adaptive_release(on != 0), {
    if (!on) live_set_release(e, e->selected().proto.compressor);
    live_reset_release_envelopes(e);
  });
}
int af_compressor_set_base_release_time(af_engine *e, double v) {
  AF_LIVE_SETTER((void)0, e->selected().proto.compressor.set_base_release_time(v),
                 if (!e->selected().proto.compressor.adaptive_release) live_set_release(e, e->selected().proto.compressor));
}
// a configuration setter: the token-ring kernel and the stage plan are built per value, and the loudness meter's rows exist only
// when it was on at the start
int af_compressor_set_auto_makeup_enabled(af_engine *e, int32_t on) { AF_SETTER(e->selected().proto.compressor.set_auto_makeup_enabled(on != 0)); }
int af_compressor_set_target_lufs(af_engine *e, double v) { AF_LIVE_PARAM_SETTER(e->selected().proto.compressor.set_target_lufs(v)); }
int af_compressor_set_sidechain_highpass_enabled(af_engine *e, int32_t on) {
  const bool changes = e && e->selected().proto.compressor.sidechain_highpass_enabled != (on != 0);
  AF_LIVE_SETTER(if (changes) AF_LIVE_SAME_PATHS_CHECK("the side-chain high-pass"),
                 e->selected().proto.compressor.set_sidechain_highpass_enabled(on != 0), {
    if (changes)  // reset_sidechain_highpass_state, compressor.rs:397-404
      for (int row : {af::kCompScPrevIn, af::kCompScPrevOut, af::kCompLowEnv, af::kCompVoicedEnv, af::kCompPresenceEnv, af::kCompPlosive})
        live_set(e, row, 0.0);
  });
}

int af_compressor_set_noise_reference_reliability(af_engine *e, double v) { AF_LIVE_PARAM_SETTER(e->selected().proto.compressor.set_noise_reference_reliability(v)); }

int af_compressor_set_activity_evidence(af_engine *e, const double *vad_probabilities, int64_t n_blocks, int32_t per_stream,
                                        double vad_reliability, double noise_floor_db, double live_noise_reliability) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (n_blocks < 0 || (n_blocks > 0 && !vad_probabilities)) return fail(AF_ERR_INVALID_ARGUMENT, "bad VAD array");
  auto unit = [](double v) { return std::isfinite(v) ? af::clampd(v, 0.0, 1.0) : 0.0; };  // compressor.rs:516-518
  e->has_evidence = n_blocks > 0;
  e->vad_reliability = unit(vad_reliability);
  e->noise_floor_db = std::isfinite(noise_floor_db) ? noise_floor_db : 1.0;  // out of [-120, 0] disables it
  e->live_noise_reliability = unit(live_noise_reliability);
  e->vad_blocks = n_blocks;
  e->params_dirty = true;
  if (e->started) {  // ChainParams carries the three scalars
    e->base().params.comp.vad_reliability = e->vad_reliability;
    e->base().params.comp.noise_floor_db = e->noise_floor_db;
    e->base().params.comp.live_noise_reliability = e->live_noise_reliability;
    e->base().params.comp.has_evidence = e->has_evidence ? 1 : 0;
  }
  if (n_blocks == 0) return AF_OK;
  AF_HIP(e->use_device());
  const int64_t total = n_blocks * e->n_streams;
  AF_HIP(e->d_vad.reserve_exact(sizeof(double) * total));
  if (per_stream) {
    AF_HIP(hipMemcpy(e->d_vad, vad_probabilities, sizeof(double) * total, hipMemcpyHostToDevice));
  } else {
    std::vector<double> expanded((size_t)total);
    for (int64_t b = 0; b < n_blocks; ++b) std::fill_n(expanded.begin() + b * e->n_streams, e->n_streams, vad_probabilities[b]);
    AF_HIP(hipMemcpy(e->d_vad, expanded.data(), sizeof(double) * total, hipMemcpyHostToDevice));
  }
  return AF_OK;
}

int af_limiter_set_ceiling(af_engine *e, double v) { AF_LIVE_PARAM_SETTER(e->selected().proto.limiter.set_ceiling(v)); }  // (limiter.rs:139-152: parameters only)
int af_limiter_set_release_time(af_engine *e, double v) { AF_LIVE_PARAM_SETTER(e->selected().proto.limiter.set_release_time(v)); }
int af_limiter_set_lookahead_ms(af_engine *e, double v) { AF_SETTER(e->selected().proto.limiter.set_lookahead_ms(v)); }
double af_limiter_ceiling_db(const af_engine *e) { return e ? e->selected().proto.limiter.ceiling_db : 0.0; }
int32_t af_limiter_lookahead_samples(const af_engine *e) { return e ? e->selected().proto.limiter.lookahead_samples : 0; }

int af_true_peak_limiter_set_release_ms(af_engine *e, float ms) { AF_LIVE_PARAM_SETTER(e->selected().proto.tp_limiter.set_release_ms(ms)); }

// Live: the de-esser's scalar settings are parameters only (deesser.rs:294-353).  Its cut frequencies move nine filters
// (set_bounds, deesser.rs:64-73): each detector filter and each dynamic EQ gets a crossfade from its live memories, and the
// dynamic EQ's crossfade runs from the stream's live coefficients to the new centre / Q at the stream's momentary gain --
// per-stream values, computed on the device into the rows at dyn_pending_row.
static void live_deesser_bounds(af_engine *e) {
  e->live_cuts.resize(e->presets.size(), 0);
  e->live_cuts[(size_t)e->current_preset] = 1;
  const af::DeEsserParams dp = e->selected().proto.deesser.params();
  for (int i = 0; i < 3; ++i) {
    const int base = af::kDeBand0 + i * af::kDeBandStride;
    for (int z_row : {base + 11, base + 15, base + 19}) live_restart_section(e, z_row);  // detector_hp, detector_lp, dynamic_eq
    live_set(e, base + 5, 0.0);  // a newly scheduled crossfade is not cancelled
    live_op(e, af::kRetunePeaking, e->dyn_pending_row + 5 * i, base + 4, dp.bands[i].dyn_cos_omega, dp.bands[i].dyn_alpha);
  }
}
#define AF_DEESSER_CUT_LIVE_CHECK                                                                                              \
  if (e->dyn_pending_row == 0) return fail(AF_ERR_BACKEND, "internal: live control is on but the pending-coefficient rows are missing")
int af_deesser_set_auto_enabled(af_engine *e, int32_t on) { AF_LIVE_PARAM_SETTER(e->selected().proto.deesser.auto_enabled = on != 0); }
int af_deesser_set_auto_amount(af_engine *e, double v) { AF_LIVE_PARAM_SETTER(e->selected().proto.deesser.set_auto_amount(v)); }
int af_deesser_set_low_cut_hz(af_engine *e, double v) { AF_LIVE_SETTER(AF_DEESSER_CUT_LIVE_CHECK, e->selected().proto.deesser.set_low_cut_hz(v), live_deesser_bounds(e)); }
int af_deesser_set_high_cut_hz(af_engine *e, double v) { AF_LIVE_SETTER(AF_DEESSER_CUT_LIVE_CHECK, e->selected().proto.deesser.set_high_cut_hz(v), live_deesser_bounds(e)); }
int af_deesser_set_threshold_db(af_engine *e, double v) { AF_LIVE_PARAM_SETTER(e->selected().proto.deesser.set_threshold_db(v)); }
int af_deesser_set_ratio(af_engine *e, double v) { AF_LIVE_PARAM_SETTER(e->selected().proto.deesser.set_ratio(v)); }
int af_deesser_set_attack_ms(af_engine *e, double v) { AF_LIVE_PARAM_SETTER(e->selected().proto.deesser.set_attack_ms(v)); }
int af_deesser_set_release_ms(af_engine *e, double v) { AF_LIVE_PARAM_SETTER(e->selected().proto.deesser.set_release_ms(v)); }
int af_deesser_set_max_reduction_db(af_engine *e, double v) { AF_LIVE_PARAM_SETTER(e->selected().proto.deesser.set_max_reduction_db(v)); }

// ---- RNNoise suppressor (rust-core/src/dsp/rnnoise.rs) ----
int af_engine_set_suppressor_enabled(af_engine *e, int32_t on) { AF_SETTER(e->supp.enabled = on != 0); }
int af_engine_set_suppressor_strength(af_engine *e, float strength) {  // rnnoise.rs:67-72; allowed while streaming
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  e->supp.strength = af::clampf(strength, 0.0f, 1.0f);
  return AF_OK;
}
// ---- noise gate stage: live between calls, like the realtime apply_gate_control (processor/control.rs:851-865); the
// ranges are the realtime processor's (audio/processor.rs:77-82), a non-finite value leaves the setting as it is
// (clamp_control_value, control.rs:50-52)
namespace {
void gate_control(double v, double lo, double hi, double *dst) {
  if (std::isfinite(v)) *dst = v < lo ? lo : (v > hi ? hi : v);
}
}  // namespace
int af_engine_set_gate_enabled(af_engine *e, int32_t on) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  e->gate_enabled = on != 0;
  return AF_OK;
}
int32_t af_engine_gate_enabled(const af_engine *e) { return e && e->gate_enabled ? 1 : 0; }
int af_gate_set_threshold(af_engine *e, double threshold_db) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  gate_control(threshold_db, -80.0, -10.0, &e->gate_threshold_db);
  return AF_OK;
}
int af_gate_set_attack_time(af_engine *e, double attack_ms) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  gate_control(attack_ms, 0.1, 100.0, &e->gate_attack_ms);
  return AF_OK;
}
int af_gate_set_release_time(af_engine *e, double release_ms) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  gate_control(release_ms, 10.0, 1000.0, &e->gate_release_ms);
  return AF_OK;
}
int af_gate_set_mode(af_engine *e, int32_t mode) {  // gate_controls.rs:75-81; gate.rs:812-821
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (mode < 0 || mode > 2) return fail(AF_ERR_INVALID_ARGUMENT, "Invalid gate mode");
  e->gate_mode = mode;
  if (mode == 0) drop_vad_evidence(e);  // (as on a detach: no fused call can follow until the mode changes again)
  if (mode == 0 && e->d_gate) {  // set_gate_mode(ThresholdOnly) clears the auto-relax counter at once
    AF_HIP(e->use_device());
    AF_HIP(hipDeviceSynchronize());
    AF_HIP(hipMemset(e->d_gate + (int64_t)af::kGateRelax * e->n_streams, 0, sizeof(int64_t) * e->n_streams));
    // ... and puts gate_state back to Closed (gate.rs:814-815)
    if (e->d_gate_vad)
      AF_HIP(hipMemset(e->d_gate_vad + (int64_t)af::kVadGateState * e->n_streams, 0, sizeof(uint32_t) * e->n_streams));
  }
  return AF_OK;
}
double af_gate_threshold_db(const af_engine *e) { return e ? e->gate_threshold_db : 0.0; }
// ---- the VAD-fused modes: NoiseGate::set_vad_auto_gate (gate.rs:829-836) and the controller's live controls
// (apply_gate_control, control.rs:856-864, over vad.rs:984, 1002, 1043, 1054)
namespace {
void vad_control(double v, float lo, float hi, float *dst) {
  if (std::isfinite(v)) *dst = (float)v < lo ? lo : ((float)v > hi ? hi : (float)v);
}
}  // namespace
int af_gate_set_vad_auto_gate_enabled(af_engine *e, int32_t on) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if ((on != 0) == e->gate_vad_attached) return AF_OK;
  e->gate_vad_attached = on != 0;
  if (!on) drop_vad_evidence(e);  // evidence is for a fused call: none can follow until the controller is back
  if (on) e->vad_ctl_fresh = true;  // a newly attached controller starts from VadAutoGate::without_backend's state
  return AF_OK;
}
int af_gate_set_vad_threshold(af_engine *e, double threshold) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  vad_control(threshold, 0.0f, 1.0f, &e->vad_threshold);
  return AF_OK;
}
int af_gate_set_hold_time(af_engine *e, double hold_ms) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  vad_control(hold_ms, 0.0f, 500.0f, &e->vad_hold_ms);
  return AF_OK;
}
int af_gate_set_margin(af_engine *e, double margin_db) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  vad_control(margin_db, 0.0f, 20.0f, &e->vad_margin_db);
  return AF_OK;
}
int af_gate_set_auto_threshold(af_engine *e, int32_t on) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  e->vad_auto_threshold = on != 0;  // (vad.rs:1005-1008 repairs a floor <= -100 dB, which the clamp at :747 never lets arise)
  return AF_OK;
}
int af_gate_read_vad_controls(const af_engine *e, double *vad_threshold, double *hold_ms, double *margin_db, int32_t *auto_threshold,
                              int32_t *attached) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (vad_threshold) *vad_threshold = e->vad_threshold;
  if (hold_ms) *hold_ms = e->vad_hold_ms;
  if (margin_db) *margin_db = e->vad_margin_db;
  if (auto_threshold) *auto_threshold = e->vad_auto_threshold ? 1 : 0;
  if (attached) *attached = e->gate_vad_attached ? 1 : 0;
  return AF_OK;
}
int af_gate_set_vad_evidence(af_engine *e, const float *probabilities, const uint8_t *available, int64_t n_blocks, int32_t per_stream) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (n_blocks < 0 || (n_blocks > 0 && (!probabilities || !available))) return fail(AF_ERR_INVALID_ARGUMENT, "bad VAD evidence arrays");
  const size_t count = (size_t)n_blocks * (per_stream ? (size_t)e->n_streams : 1);
  e->vad_ev_prob.assign(probabilities, probabilities + count);
  for (float &p : e->vad_ev_prob) p = std::isfinite(p) ? p : 0.0f;  // (the clamp to [0, 1] is the control pass's, gate.rs:841)
  e->vad_ev_avail.assign(available, available + count);
  e->vad_ev_blocks = n_blocks;
  e->vad_ev_per_stream = per_stream != 0;
  return AF_OK;
}
int af_engine_read_gate_vad_decisions(af_engine *e, float *probability, float *noise_floor_db, int32_t *flags, int64_t n_blocks) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (n_blocks != e->vad_dec_blocks)
    return fail(AF_ERR_INVALID_ARGUMENT, "the last fused call left %lld decision rows, not %lld", (long long)e->vad_dec_blocks,
                (long long)n_blocks);
  if (n_blocks == 0) return AF_OK;
  const int64_t NS = e->n_streams;
  std::vector<uint32_t> rows((size_t)(n_blocks * af::kVadDecWords * NS));
  AF_HIP(e->use_device());
  AF_HIP(hipDeviceSynchronize());
  AF_HIP(hipMemcpy(rows.data(), e->d_vad_dec, sizeof(uint32_t) * rows.size(), hipMemcpyDeviceToHost));
  for (int64_t b = 0; b < n_blocks; ++b)
    for (int64_t s = 0; s < NS; ++s) {
      const uint32_t *row = rows.data() + b * af::kVadDecWords * NS + s;
      if (probability) std::memcpy(&probability[b * NS + s], &row[af::kVadDecProb * NS], sizeof(float));
      if (noise_floor_db) std::memcpy(&noise_floor_db[b * NS + s], &row[af::kVadDecFloor * NS], sizeof(float));
      if (flags) flags[b * NS + s] = ((row[af::kVadDecFlags * NS] & af::kVadDecHeld) ? 1 : 0) | ((row[af::kVadDecFlags * NS] & af::kVadDecAvail) ? 4 : 0);
    }
  return AF_OK;
}
int af_engine_read_gate_vad_state(af_engine *e, float *noise_floor_db, float *noise_floor_reliability, float *fused_score,
                                  float *probability, int32_t *gate_state, int32_t *flags, int32_t n_streams) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (n_streams < 0 || n_streams > e->n_streams)
    return fail(AF_ERR_INVALID_ARGUMENT, "n_streams %d is outside [0, %d]", n_streams, e->n_streams);
  const int64_t NS = e->n_streams;
  std::vector<uint32_t> rows;
  const bool ctl_live = e->d_gate_vad && !e->vad_ctl_fresh, fused_live = e->d_gate_vad && !e->vad_fused_fresh;
  if (ctl_live || fused_live) {
    rows.resize((size_t)(af::kVadFields * NS));
    AF_HIP(e->use_device());
    AF_HIP(hipDeviceSynchronize());
    AF_HIP(hipMemcpy(rows.data(), e->d_gate_vad, sizeof(uint32_t) * rows.size(), hipMemcpyDeviceToHost));
  }
  auto word = [&](int field, int32_t s) { return rows[(size_t)(field * NS + s)]; };
  auto f32 = [&](int field, int32_t s) { float v; const uint32_t w = word(field, s); std::memcpy(&v, &w, sizeof v); return v; };
  for (int32_t s = 0; s < n_streams; ++s) {
    float floor_db = -60.0f, reliability = 0.0f, score = 0.0f, prob = 0.0f;  // gate.rs:935-951 without a controller
    int32_t state = 0, fl = 0;
    if (ctl_live && e->gate_vad_attached) {
      floor_db = f32(af::kVadFloor, s);
      // noise_floor_reliability, vad.rs:805-821 over noise_floor_percentile :786-802
      const int len = (int)word(af::kVadHistLen, s);
      if (len > 0) {
        auto percentile = [&](float pct) {
          size_t target = (size_t)std::floor((float)len * pct);
          target = std::min<size_t>(target, (size_t)len - 1);
          size_t cumulative = 0;
          for (int b = 0; b < af::kVadBinCount; ++b) {
            cumulative += word(af::kVadBins + b, s);
            if (cumulative > target) return -80.0f + (float)b * 1.0f;
          }
          return floor_db;
        };
        const float maturity = std::min(std::max((float)len / (float)af::kVadHistory, 0.0f), 1.0f);
        const float spread = std::max(percentile(0.80f) - percentile(0.20f), 0.0f);
        const float t = std::min(std::max((spread - 3.0f) / 7.0f, 0.0f), 1.0f);
        const float stationarity = 1.0f - t * t * (3.0f - 2.0f * t);
        reliability = std::min(std::max(maturity * stationarity, 0.0f), 1.0f);
      }
      fl |= (word(af::kVadLastFlags, s) & af::kVadDecHeld) ? 1 : 0;
      fl |= (word(af::kVadLastFlags, s) & af::kVadDecAvail) ? 4 : 0;
    }
    if (fused_live) {
      score = f32(af::kVadFusedScore, s);
      prob = f32(af::kVadSmoothed, s);
      state = (int32_t)word(af::kVadGateState, s);
      fl |= word(af::kVadFusedOpen, s) ? 2 : 0;
    }
    if (noise_floor_db) noise_floor_db[s] = floor_db;
    if (noise_floor_reliability) noise_floor_reliability[s] = reliability;
    if (fused_score) fused_score[s] = score;
    if (probability) probability[s] = prob;
    if (gate_state) gate_state[s] = state;
    if (flags) flags[s] = fl;
  }
  return AF_OK;
}
int af_engine_read_gate_state(af_engine *e, float *current_gain, uint64_t *chatter_events, int32_t *flags, int32_t n_streams) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (n_streams < 0 || n_streams > e->n_streams)
    return fail(AF_ERR_INVALID_ARGUMENT, "n_streams %d is outside [0, %d]", n_streams, e->n_streams);
  const int64_t NS = e->n_streams;
  std::vector<int64_t> rows;
  if (e->d_gate) {
    rows.resize((size_t)(af::kGateFields * NS));
    AF_HIP(e->use_device());
    AF_HIP(hipDeviceSynchronize());
    AF_HIP(hipMemcpy(rows.data(), e->d_gate, sizeof(int64_t) * rows.size(), hipMemcpyDeviceToHost));
  }
  for (int32_t s = 0; s < n_streams; ++s) {
    double gain = 0.0;
    int64_t events = 0, open = 0, relax = 0;
    if (!rows.empty()) {
      std::memcpy(&gain, &rows[(size_t)(af::kGateGain * NS + s)], sizeof(double));
      events = rows[(size_t)(af::kGateEvents * NS + s)];
      open = rows[(size_t)(af::kGateOpen * NS + s)];
      relax = rows[(size_t)(af::kGateRelax * NS + s)];
    }
    if (current_gain) current_gain[s] = (float)gain;  // NoiseGate::current_gain
    if (chatter_events) chatter_events[s] = (uint64_t)events;
    if (flags) flags[s] = (open ? 1 : 0) | (relax > 0 ? 2 : 0);
  }
  return AF_OK;
}

int af_suppressor_set_raw_protocol(af_engine *e, int32_t on) { AF_SETTER(e->supp.raw_protocol = on != 0); }
int af_suppressor_set_synthetic_weights(af_engine *e, uint64_t seed) {
  AF_SETTER((af::synthetic_weights(e->supp.weights, seed), e->supp.weights_dirty = true));
}
int af_suppressor_load_weights(af_engine *e, const int8_t *blob, size_t bytes) {
  if (!blob || bytes != sizeof(af::RnnWeightsI8))
    return fail(AF_ERR_INVALID_ARGUMENT, "weight blob must be %zu bytes (the fifteen int8 arrays of the RNNoise model)",
                sizeof(af::RnnWeightsI8));
  AF_SETTER((std::memcpy(&e->supp.weights, blob, bytes), e->supp.weights_dirty = true));
}
int32_t af_suppressor_latency_samples(const af_engine *) { return af::kRnnFrame; }  // rnnoise.rs:313-315
// test tap: one (frame, stream) record of buffer set 0: Ex Ep Exp feat[44] gains_raw gains silence pitch, then X, P.  Set 0 holds
// the call's last window only when the call had at most one window per set: valid after a one-window call, as every test uses it.
int af_suppressor_debug_read(af_engine *e, int32_t frame, int32_t stream, float *rec_out, float *x_out, float *p_out) {
  if (!e || !e->supp.d_rec) return fail(AF_ERR_STATE, "no suppressor window has run");
  if (frame < 0 || frame >= e->supp.ws_frames || stream < 0 || stream >= e->n_streams)
    return fail(AF_ERR_INVALID_ARGUMENT, "frame/stream out of range");
  AF_HIP(e->use_device());
  AF_HIP(hipDeviceSynchronize());
  const size_t cell = (size_t)frame * e->n_streams + stream;
  af::SuppArgs set0{};
  e->supp.window_buffers(set0, 0, 1, 0);
  AF_HIP(hipMemcpy(rec_out, set0.rec + cell, sizeof(af::SuppFrameRec), hipMemcpyDeviceToHost));
  if (x_out) AF_HIP(hipMemcpy(x_out, set0.X + cell * af::kRnnFreq, sizeof(float2) * af::kRnnFreq, hipMemcpyDeviceToHost));
  if (p_out) AF_HIP(hipMemcpy(p_out, set0.P + cell * af::kRnnFreq, sizeof(float2) * af::kRnnFreq, hipMemcpyDeviceToHost));
  return AF_OK;
}
// test tap of the pitch path: the whitened pitch buffer of one (frame, stream) cell of the LAST window (`d_ds` is a single set),
// and the stream's tracker state (last period, last gain) as the last call left it
int af_suppressor_debug_read_pitch(af_engine *e, int32_t frame, int32_t stream, float *whitened, int32_t *last_period, float *last_gain) {
  if (!e || !e->supp.d_ds || !e->supp.d_state) return fail(AF_ERR_STATE, "no suppressor window has run");
  if (stream < 0 || stream >= e->n_streams || (whitened && (frame < 0 || frame >= e->supp.ws_frames)))
    return fail(AF_ERR_INVALID_ARGUMENT, "frame/stream out of range");
  AF_HIP(e->use_device());
  AF_HIP(hipDeviceSynchronize());
  float ds[af::kPitchBuf / 2], state[2];
  af::SuppArgs bufs{};
  e->supp.window_buffers(bufs, 0, 1, 0);
  static_assert(af::SuppState::kLastGain == af::SuppState::kLastPeriod + 1, "last period and gain are neighbours");
  if (whitened) {
    const size_t cell = (size_t)frame * e->n_streams + stream;
    AF_HIP(hipMemcpy(ds, bufs.ds + cell * (af::kPitchBuf / 2), sizeof ds, hipMemcpyDeviceToHost));
  }
  AF_HIP(hipMemcpy(state, bufs.state + (size_t)stream * af::SuppState::kCount + af::SuppState::kLastPeriod, sizeof state,
                   hipMemcpyDeviceToHost));
  if (whitened) std::memcpy(whitened, ds, sizeof ds);  // (outputs are written only once every copy has succeeded)
  if (last_period) *last_period = (int32_t)state[0];
  if (last_gain) *last_gain = state[1];
  return AF_OK;
}
// test tap of the pre-pass: one stream's row of the LAST window's model-input buffer -- the 1728 history samples the pre-pass
// copied in front, then the window's samples -- and the row's length
int af_suppressor_debug_read_model_input(af_engine *e, int32_t stream, float *row, int64_t capacity, int64_t *length) {
  if (!e || !e->supp.d_xh || e->supp.last_xh_slot < 0) return fail(AF_ERR_STATE, "no suppressor window has run");
  const int64_t n = af::kPitchBuf + (int64_t)e->supp.last_xh_frames * af::kRnnFrame;
  if (stream < 0 || stream >= e->n_streams || !length || (row && capacity < n))
    return fail(AF_ERR_INVALID_ARGUMENT, "stream out of range, no length pointer, or fewer than %lld floats of room", (long long)n);
  if (row) {
    AF_HIP(e->use_device());
    AF_HIP(hipDeviceSynchronize());
    af::SuppArgs last{};
    e->supp.window_buffers(last, e->supp.last_xh_slot, 1, 0);  // (a slot is its own index modulo the buffer count)
    AF_HIP(hipMemcpy(row, last.xh + (size_t)stream * (size_t)n, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
  }
  *length = n;
  return AF_OK;
}
// test tap: ONLY the pitch search kernel, through the launcher the engine uses, on caller-supplied model-input spans
// [stream][1728 + 480 n_frames] (host pointers): its whitened buffers [frame][stream][864] and its own pitch index
// [frame][stream] -- the one the tracker overwrites in an engine run.  No engine, no state.
int af_suppressor_debug_pitch_search(const float *spans, int32_t n_streams, int32_t n_frames, float *whitened, int32_t *pitch_index,
                                     int32_t device) {
  if (!spans || !whitened || !pitch_index) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (n_streams < 1 || n_streams > 4096 || n_frames < 1 || n_frames > 64)
    return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be in [1, 4096] and n_frames in [1, 64]");
  AF_HIP(hipSetDevice(device));
  const size_t cells = (size_t)n_frames * n_streams;
  const size_t span_floats = (size_t)n_streams * (af::kPitchBuf + (size_t)n_frames * af::kRnnFrame);
  af::DeviceBuffer<float> d_xh, d_ds;
  af::DeviceBuffer<af::SuppFrameRec> d_rec;
  AF_HIP(d_xh.reserve_exact(sizeof(float) * span_floats));
  AF_HIP(d_ds.reserve_exact(sizeof(float) * cells * (af::kPitchBuf / 2)));
  AF_HIP(d_rec.reserve_exact(sizeof(af::SuppFrameRec) * cells));
  std::vector<float> ds(cells * (af::kPitchBuf / 2));
  std::vector<af::SuppFrameRec> rec(cells);
  af::SuppArgs sa{};
  sa.xh = d_xh;
  sa.ds = d_ds;
  sa.rec = d_rec;
  sa.n_streams = n_streams;
  sa.n_frames = n_frames;
  hipError_t err = hipMemcpy(d_xh, spans, sizeof(float) * span_floats, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemset(d_ds, 0xFF, sizeof(float) * ds.size());  // (a cell the kernel leaves out reads as NaN)
  if (err == hipSuccess) err = hipMemset(d_rec, 0xFF, sizeof(af::SuppFrameRec) * cells);
  if (err == hipSuccess) err = af::launch_suppressor_pitch_search(sa, af::SuppTables{}, nullptr);  // (the search reads no table)
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(ds.data(), d_ds, sizeof(float) * ds.size(), hipMemcpyDeviceToHost);
  if (err == hipSuccess) err = hipMemcpy(rec.data(), d_rec, sizeof(af::SuppFrameRec) * cells, hipMemcpyDeviceToHost);
  if (err != hipSuccess) return fail(AF_ERR_BACKEND, "pitch search probe failed: %s", hipGetErrorString(err));
  std::memcpy(whitened, ds.data(), sizeof(float) * ds.size());
  for (size_t c = 0; c < cells; ++c) pitch_index[c] = rec[c].pitch_index;
  return AF_OK;
}

// ---- presets: several chain configurations in one engine, one per 64-stream group
int af_engine_set_preset_count(af_engine *e, int32_t n) {
  if (n < 1 || n > 256) return fail(AF_ERR_INVALID_ARGUMENT, "preset count must be in [1, 256]");
  if (int rc = require_config(e)) return rc;
  while (e->n_presets() > n) e->presets.pop_back();
  while (e->n_presets() < n) {  // a fresh OfflineDspBlockProcessor::new(sample_rate), block_processor.rs:46-60
    e->presets.emplace_back(e->base().proto.sample_rate);  // (may reallocate: base() is taken anew below)
    af::ChainProto &np = e->presets.back().proto;
    const af::ChainProto &p0 = e->base().proto;
    np.control_block = p0.control_block;
    np.input_scrub = p0.input_scrub;
    np.input_clamp = p0.input_clamp;
    np.dc_block = p0.dc_block;
    np.pre_highpass = p0.pre_highpass;
  }
  if (e->current_preset >= n) e->current_preset = 0;
  for (int32_t &g : e->group_preset)
    if (g >= n) g = 0;
  return AF_OK;
}
int32_t af_engine_preset_count(const af_engine *e) { return e ? e->n_presets() : 0; }
int af_engine_select_preset(af_engine *e, int32_t preset) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (preset < 0 || preset >= e->n_presets()) return fail(AF_ERR_INVALID_ARGUMENT, "preset %d does not exist", preset);
  e->current_preset = preset;
  return AF_OK;
}
int af_engine_assign_presets(af_engine *e, const int32_t *preset_of_group, int32_t n_groups) {
  if (!e || !preset_of_group) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (n_groups != (e->n_streams + 63) / 64)
    return fail(AF_ERR_INVALID_ARGUMENT, "expected one preset index per group of 64 streams (%d), got %d", (e->n_streams + 63) / 64, n_groups);
  for (int32_t g = 0; g < n_groups; ++g)
    if (preset_of_group[g] < 0 || preset_of_group[g] >= e->n_presets())
      return fail(AF_ERR_INVALID_ARGUMENT, "group %d: preset %d does not exist", g, preset_of_group[g]);
  if (int rc = require_config(e)) return rc;
  e->group_preset.assign(preset_of_group, preset_of_group + n_groups);
  return AF_OK;
}

int af_engine_set_kernel(af_engine *e, int32_t kernel) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (kernel < AF_KERNEL_AUTO || kernel > AF_KERNEL_ROLES) return fail(AF_ERR_INVALID_ARGUMENT, "unknown kernel id %d", kernel);
  e->kernel = kernel;
  return AF_OK;
}
int af_engine_set_ring_variant(af_engine *e, int32_t waves, int32_t chunk) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  const int v = waves * 100 + chunk;
  if (v != 0 && v != 1604 && v != 1602 && v != 804 && v != 802 && v != 1204 && v != 1202)
    return fail(AF_ERR_INVALID_ARGUMENT, "no token-ring kernel is built for %d waves x %d-sample chunks", waves, chunk);
  e->ring_variant = v;
  return AF_OK;
}
int af_engine_last_kernel(const af_engine *e) { return e ? e->last_kernel_used : 0; }
int af_engine_debug_detector_reuse_chunks(af_engine *e, uint64_t *chunks) {
  if (!e || !chunks) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  *chunks = 0;
  if (!e->d_status) return AF_OK;  // nothing has run yet
  AF_HIP(e->use_device());
  AF_HIP(hipDeviceSynchronize());
  unsigned long long n = 0;
  AF_HIP(hipMemcpy(&n, e->d_status.get() + af::kStatusReuseWord, sizeof n, hipMemcpyDeviceToHost));
  *chunks = (uint64_t)n;
  return AF_OK;
}
int af_engine_set_timing_enabled(af_engine *e, int32_t on) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  e->timing = on != 0;
  return AF_OK;
}

// a call that runs n_run samples per stream needs evidence, where evidence is pending, for exactly its control blocks
static int check_evidence_blocks(const af_engine *e, int64_t n_run) {
  const int cb = e->base().params.control_block;
  const int64_t blocks = (n_run + cb - 1) / cb;
  if (n_run > 0 && (e->base().params.flags & af::kFlagCompressor) && e->base().params.comp.auto_makeup_enabled && e->has_evidence &&
      e->vad_blocks != blocks)
    return fail(AF_ERR_INVALID_ARGUMENT, "expected %lld VAD probabilities at the control cadence, got %lld",
                (long long)blocks, (long long)e->vad_blocks);
  if (n_run > 0 && gate_vad_fused(e) && e->vad_ev_blocks > 0 && e->vad_ev_blocks != blocks)
    return fail(AF_ERR_INVALID_ARGUMENT, "expected %lld VAD evidence blocks at the control cadence, got %lld", (long long)blocks,
                (long long)e->vad_ev_blocks);
  return AF_OK;
}

static bool io_resampled(const af_engine *e) { return e->rs_in || e->rs_out; }
static const char *const kStreamOnlyMessage =
    "this engine resamples its input or output (af_engine_set_io_sample_rates): use af_engine_stream_host";
static const char *const kWriterStreamOnlyMessage =
    "this engine runs the output writer (af_engine_set_output_writer): use af_engine_stream_host";
static const char *const kChannelsStreamOnlyMessage =
    "this engine takes multichannel input (af_engine_set_input_channels): use af_engine_stream_host";

// ---- what the three paths of a process call share
// one accepted call's arguments, as the paths below take them
struct CallArgs {
  const float *chain_in;  // what the chain reads: the caller's `in`, or `out` behind the noise gate's pre-pass
  float *out;
  int64_t n_samples, stream_stride;
  int32_t layout;
  hipStream_t stream;
  uint32_t gate_strip;  // the front-end flags the noise gate's pre-pass has taken over (0: there was none)
  int64_t rows;         // statistics rows of the call: control blocks x streams
};

static_assert(af::kRnnFrame == 480, "af::supp_window_unit counts 480-sample frames");
static int64_t whole_blocks(int cb, int64_t samples) { return (int64_t)cb * std::max<int64_t>(1, samples / cb); }
constexpr int64_t kStageWindowSamples = 2880;  // the stage pipeline's window behind the suppressor (Switches::stage_window without it)

static bool eq_crossfade_pending(const af::ChainParams &hp) {
  bool xf = false;
  for (int j = 0; j < hp.n_eq_sections; ++j) xf = xf || hp.eq[j].xf_remaining > 0;
  return xf;
}

// Whether the chain of `hp` can run with its EQ launched beside it (af_eq_systolic.hip) and the rest as the plain one-launch
// form of the token-ring kernel.  `also_barred`: flags that keep this caller off the form besides the de-esser and the
// sample-serial front end; `crossfade_lds`: size the launch's LDS for a coefficient crossfade.
static bool eq_side_launch_serves(const af::ChainParams &hp, uint32_t also_barred, bool crossfade_lds) {
  return !(hp.flags & (af::kFlagDeesser | af::kFlagDcBlock | af::kFlagPreHighpass | also_barred)) && hp.n_eq_sections <= 16 &&
         af::ring_kernel_dynamic_lds(hp.n_eq_sections, hp.lim.lookahead_samples, crossfade_lds) <= af::kMaxLdsBytes;
}

// window number `index` of this call in the stage pipeline: `n` samples from sample `t0` of the call, its rows from `blocks_at`
static af::DiagWin diag_window(const af_engine *e, int64_t index, int64_t t0, int64_t n, int64_t blocks_at, const float *in, float *out) {
  af::DiagWin wd{};
  wd.n0 = e->samples_processed + t0;
  wd.n = n;
  wd.stats = e->d_stats + blocks_at * e->n_streams;
  wd.mk = e->pipe.d_mk + ((e->pipe.windows + index) % af_engine::StagePipe::kMkSets) * e->pipe.mk_rows;
  wd.bp = e->pipe.d_bp + ((e->pipe.windows + index) % af_engine::StagePipe::kBpSets) * e->pipe.mk_rows;
  wd.vad = e->has_evidence ? e->d_vad + blocks_at * e->n_streams : nullptr;
  wd.in = in;
  wd.out = out;
  return wd;
}

// the realtime front end (clamp + DC block + 80 Hz HP, routing.rs:802-843) as a sample-serial pre-pass runs it: which of
// `flags` it takes over, the high-pass of `hp`, the chain's state planes (`front_scrub` is the caller's)
static void supp_front_end(const af_engine *e, const af::ChainParams &hp, uint32_t flags, af::SuppArgs &sa) {
  sa.front_clamp = (flags & af::kFlagInputClamp) ? 1 : 0;
  sa.front_dc = (flags & af::kFlagDcBlock) ? 1 : 0;
  sa.front_hp = (flags & af::kFlagPreHighpass) ? 1 : 0;
  sa.hp_b0 = hp.pre_hp.b0; sa.hp_b1 = hp.pre_hp.b1; sa.hp_b2 = hp.pre_hp.b2;
  sa.hp_a1 = hp.pre_hp.a1; sa.hp_a2 = hp.pre_hp.a2;
  sa.chain_st64 = e->d_st64;
  sa.chain_st32 = e->d_st32;
  sa.f64_pre_z1 = af::kPreZ1;
  sa.f32_dc_x1 = af::kDcX1;
}

// ---- path 1: the chain as a pipeline of stage kernels over windows of whole control blocks (af_stages.hip)
// (a launch step costs ~20 us, the pipeline's fill is depth x window time: 960 samples 45.7 ms per 10 s at 256 streams,
// 1920 41.2, 2880 39.7, 4800 42.7, 9600 40.3)
static int run_stage_pipeline(af_engine *e, const CallArgs &c) {
  const int cb = e->base().params.control_block;
  const int64_t tw = whole_blocks(cb, af::switches().stage_window);
  if (int rc = stage_pipe_prepare(e, std::max<int64_t>(tw, e->pipe.tw_max))) return rc;
  e->pipe.strip = e->base().params.flags & c.gate_strip;
  if (int rc = stage_chain_params(e, c.stream)) return rc;  // what the stage kernels read (everything but the EQ sections)
  e->last_kernel_used = AF_KERNEL_STAGED;
  // one launch step per window on the caller's stream: step j runs every stage on the window it has reached
  const StagePlan plan = stage_plan(e->base().params);
  std::vector<af::DiagWin> wins;
  int64_t blocks_at = 0;
  for (int64_t t0 = 0; t0 < c.n_samples; t0 += tw) {
    const int64_t n_w = std::min<int64_t>(tw, c.n_samples - t0);
    wins.push_back(diag_window(e, (int64_t)wins.size(), t0, n_w, blocks_at, c.chain_in + t0, c.out + t0));
    blocks_at += (n_w + cb - 1) / cb;
  }
  e->pipe.call_stride = c.stream_stride;
  AF_HIP(hipMemsetAsync(e->d_stats, 0, sizeof(af::BlockStats) * c.rows, c.stream));
  const int64_t steps = (int64_t)wins.size() + plan.depth;
  for (int64_t j = 0; j < steps; ++j) {
    if (j < (int64_t)wins.size()) {  // window j enters: its EQ stage reads the section parameters as they stand now
      bool crossfade = false;
      if (int rc = stage_diag_eq_params(e, c.stream, &crossfade, &wins[(size_t)j].eq_slot)) return rc;
      wins[(size_t)j].eq_crossfade = crossfade ? 1 : 0;
      advance_crossfades(e, wins[(size_t)j].n);
    }
    if (int rc = stage_diag_step(e, e->base().params, plan, wins, j, c.stream)) return rc;
  }
  e->pipe.windows += (int64_t)wins.size();
  return AF_OK;
}

// ---- path 2: the chain as one launch.  Large batches without the suppressor (round 3): the chain can use one CU per 64
// streams and nothing else, so the EQ -- a quarter of the token-ring kernel's time -- runs as the systolic kernel on the CUs
// the chain leaves idle, window by window, and the chain is ONE launch that follows it through the ready counter (the form
// the suppressor's pipeline uses).  Taken when the streams can be CU-partitioned and the EQ kernel serves the
// configuration; everything else is the plain segment launch on the caller's stream.
static int run_chain_launch(af_engine *e, const CallArgs &c) {
  const int cb = e->base().params.control_block;
  const hipStream_t stream = c.stream;
  af::ChainParams hp = e->base().params;  // (a copy: with the gate on, the front end is the pre-pass's)
  hp.flags &= ~c.gate_strip;
  const bool auto_mk = (hp.flags & af::kFlagCompressor) && hp.comp.auto_makeup_enabled;
  const int64_t window = whole_blocks(cb, 9600);
  // (the chain launch lays out its LDS for a crossfade only when one is pending at the call's start, as
  // launch_chain_segment sizes it: checking the crossfade layout always kept 15 and 16 sections off this form)
  bool offload = af::switches().chain_persistent && af::switches().eq_offload && (e->kernel == AF_KERNEL_AUTO || e->kernel == AF_KERNEL_PHASED) &&
                 (e->ring_variant == 0 || e->ring_variant == 1604) && e->n_presets() == 1 && af::switches().roles == 0 &&
                 c.layout == AF_LAYOUT_STREAM_MAJOR && (hp.flags & af::kFlagEq) && hp.n_eq_sections > 0 &&
                 eq_side_launch_serves(hp, af::kFlagPrePass, eq_crossfade_pending(hp)) && c.n_samples >= 2 * window &&
                 !af::switches().serial_streams;
  if (offload) {
    if (int rc = ensure_side_streams(e, stream)) return rc;
    offload = e->partition_chain_cus > 0;
  }
  if (!offload)  // (no suppressor: everything is chain time)
    return launch_chain_segment(e, hp, c.gate_strip != 0, c.chain_in, c.out, c.n_samples, c.stream_stride, c.layout, e->samples_processed,
                                e->d_stats, e->has_evidence ? e->d_vad : nullptr, stream, stream);
  if (auto_mk) AF_HIP(e->d_block_power.reserve_retiring(sizeof(double) * c.rows, e->retired, stream));
  AF_HIP(hipMemsetAsync(e->d_stats, 0, sizeof(af::BlockStats) * c.rows, stream));
  AF_HIP(e->d_ready.reserve_exact(sizeof(int64_t)));
  AF_HIP(hipMemsetAsync(e->d_ready, 0, sizeof(int64_t), stream));
  hipEvent_t ev;
  if (int rc = engine_event(e, &ev)) return rc;
  AF_HIP(hipEventRecord(ev, stream));
  AF_HIP(hipStreamWaitEvent(e->aux_stream, ev, 0));
  AF_HIP(hipStreamWaitEvent(e->eq_stream, ev, 0));
  af::ChainParams run_p = hp;  // the EQ kernel scrubs / clamps the input and keeps the block input statistics
  run_p.flags = (run_p.flags & ~(af::kFlagEq | af::kFlagInputScrub | af::kFlagInputClamp)) | af::kFlagInputDone;
  if (int rc = launch_chain_segment(e, run_p, true, c.out, c.out, c.n_samples, c.stream_stride, c.layout, e->samples_processed, e->d_stats,
                                    e->has_evidence ? e->d_vad : nullptr, e->aux_stream, stream, /*stats_cleared=*/true,
                                    auto_mk ? e->d_block_power : nullptr, e->d_ready))
    return rc;
  int64_t blocks_done = 0;
  for (int64_t seg0 = 0; seg0 < c.n_samples; seg0 += window) {
    const int64_t seg_n = std::min<int64_t>(window, c.n_samples - seg0);
    const std::vector<af::ChainParams> run_eq = run_params(e, c.gate_strip);  // (as the crossfade counters stand at this window)
    AF_HIP(e->d_params_eq.sync(run_eq.data(), run_eq.size(), e->stager, e->eq_stream));
    AF_HIP(af::launch_eq_systolic(e->d_params_eq, nullptr, e->d_st64, c.chain_in + seg0, c.out + seg0, nullptr, nullptr, 0, 0,
                                  e->d_stats + blocks_done * e->n_streams, eq_crossfade_pending(run_eq[0]), seg_n, c.stream_stride, e->n_streams,
                                  e->eq_stream,
                                  auto_mk ? e->d_block_power + blocks_done * e->n_streams : nullptr));  // (the systolic form: here the EQ's own latency per window is what the chain follows)
    AF_HIP(af::launch_chain_publish_ready(e->d_ready, seg0 + seg_n, e->eq_stream));
    e->last_launches += 2;
    advance_crossfades(e, seg_n);
    blocks_done += (seg_n + cb - 1) / cb;
  }
  for (hipStream_t side : {e->aux_stream.get(), e->eq_stream.get()}) {
    if (int rc = engine_event(e, &ev)) return rc;
    AF_HIP(hipEventRecord(ev, side));
    AF_HIP(hipStreamWaitEvent(stream, ev, 0));
  }
  return AF_OK;
}

// ---- path 3: the RNNoise suppressor ahead of the chain (realtime order, dsp_loop.rs:1222-1250,1521-1599).
// The call is cut into windows of frames and runs as a four-stage pipeline over them, one HIP stream each:
//   pre stream    : window w+2's sample-serial pre-pass (front end + model-input high-pass; 64 waves whose
//                   duration is set by recurrence latency, so it costs the chip almost nothing)
//   analysis      : window w+1's spectra and pitch search (the pitch kernel walks each stream's frames in
//                   order, one wave per stream: latency bound, it leaves most issue slots free)
//   caller stream : window w's pitch-aligned spectra, network, resynthesis, overlap-add
//   chain stream  : window w-1's chain launch (64 streams per workgroup, a quarter of the CUs at batch 4096)
// ordered by events; buffers that cross a stage boundary rotate (af_suppressor_host.hpp).
// `src` / `src_stride`: the call's whole frames (the caller's input or the engine's assembly buffer); `vad_args` with
// `fused_gate`: the VAD-fused gate modes' pass instead of the plain pre-pass.
static int run_suppressor_pipeline(af_engine *e, const CallArgs &c, const float *src, int64_t src_stride, bool fused_gate,
                                   const af::VadGateArgs &vad_args) {
  const af::Switches &sw = af::switches();
  const int cb = e->base().params.control_block;
  const hipStream_t stream = c.stream;
  float *const out = c.out;
  const int64_t stream_stride = c.stream_stride;
  if (e->supp.weights_dirty) AF_HIP(e->supp.upload());
  af::ChainParams run = e->base().params;
  bool run_modified = false;
  const uint32_t front = af::kFlagInputClamp | af::kFlagDcBlock | af::kFlagPreHighpass;
  const uint32_t front_flags = run.flags & front;
  const bool strip_front = front_flags || e->gate_enabled;  // the gate runs in the pre-pass too, after the front end
  if (strip_front) {
    // the realtime front end runs inside the suppressor's own sample-serial pre-pass, so the chain launches must not repeat it
    run.flags &= ~(front | af::kFlagInputScrub);
    run_modified = true;
  }
  const int64_t frames = c.n_samples / af::kRnnFrame;
  const std::vector<af::SuppWindow> wins = af::supp_window_schedule(frames, af::supp_window_unit(cb), e->supp_window_frames, e->pipe.active, sw);
  {
    int64_t longest = 1;
    for (const af::SuppWindow &win : wins) longest = std::max(longest, win.nf);
    AF_HIP(e->supp.ensure_workspace(e->n_streams, (int)longest));
  }
  if (e->trace) {
    if (sizeof(int32_t) * 2 * frames * e->n_streams > e->d_trace.bytes()) {
      AF_HIP(hipDeviceSynchronize());
      AF_HIP(e->d_trace.reserve_exact(sizeof(int32_t) * 2 * frames * e->n_streams));
    }
    e->trace_frames = frames;
  }
  // (a suppressor window enters the stage pipeline in pieces of the pipeline's own window length: the rings stay as small as
  // without the suppressor)
  const int64_t chain_tw = whole_blocks(cb, kStageWindowSamples);
  if (e->pipe.active) {
    if (int rc = stage_pipe_prepare(e, std::max<int64_t>(chain_tw, e->pipe.tw_max))) return rc;
    e->pipe.strip = e->base().params.flags & ~run.flags;  // what the pre-pass has taken over
    if (int rc = stage_chain_params(e, stream)) return rc;  // (everything but the EQ sections is read from here)
  }
  if (int rc = ensure_side_streams(e, stream)) return rc;
  const hipStream_t fin = sw.synth_split ? e->fin_stream : nullptr;
  const hipStream_t syn = e->syn_stream ? e->syn_stream : stream;  // where the synthesis stage runs
  const hipStream_t last_supp = (fin && fin != syn) ? fin : syn;   // where a window's last suppressor kernel runs
  int64_t blocks_done = 0;
  std::vector<af::DiagWin> diag_wins;                 // the call's windows in the stage pipeline (one launch per step)
  const StagePlan diag_plan = stage_plan(run);
  const bool eq_offload = sw.eq_offload && (e->kernel == AF_KERNEL_AUTO || e->kernel == AF_KERNEL_PHASED || e->kernel == AF_KERNEL_ROLES) &&
                          (e->ring_variant == 0 || e->ring_variant == 1604) && (run.flags & af::kFlagEq);
  bool eq_needs_chain_done = true;  // (the previous call's last chain launch has ended: the caller's stream waited for it)
  const bool auto_makeup_call = (run.flags & af::kFlagCompressor) && run.comp.auto_makeup_enabled;
  if (eq_offload && auto_makeup_call && !e->pipe.active) {
    // the systolic EQ kernel is then also the pre-pass of every window (it leaves the compressor-input block powers here)
    AF_HIP(e->d_block_power.reserve_retiring(sizeof(double) * c.rows, e->retired, stream));
  }
  auto next_event = [&](hipEvent_t *out_ev) -> int { return engine_event(e, out_ev); };
  // The call's statistics rows are cleared ONCE, here (their fields are written by the kernels that own them).  Round 2 cleared
  // every window's rows in front of its EQ launch: a fill kernel on the suppressor's crowded CUs, 0.05-0.45 ms between the
  // window's overlap-add and its EQ -- on the path the first chain launches wait for.
  AF_HIP(hipMemsetAsync(e->d_stats, 0, sizeof(af::BlockStats) * c.rows, stream));
  // ---- ONE chain launch per call (round 3).  With the chain's CUs its own, the EQ on the suppressor's side and nothing that
  // changes the parameter block between windows, the token-ring kernel is launched once, for the whole call, before the first
  // window: a chunk waits until the counter `d_ready` covers its samples, and every window's EQ launch is followed by a
  // one-thread kernel that publishes the new count.  What that removes from the chain's stream: 53 dispatches and their
  // cross-stream dependencies (~0.1 ms each while six other queues are busy: the trace of tools/step_timeline.py), the
  // state planes' load and write-back per window, and the fill / drain of the 16-wave pipeline per launch.
  // AF_CHAIN_PERSISTENT=0 restores one launch per window (A/B runs).
  const bool persistent = sw.chain_persistent && eq_offload && e->partition_chain_cus > 0 && !e->pipe.active && !sw.diag_skip_chain &&
                          e->n_presets() == 1 && sw.roles == 0 && (e->kernel == AF_KERNEL_AUTO || e->kernel == AF_KERNEL_PHASED) &&
                          c.layout == AF_LAYOUT_STREAM_MAJOR && eq_side_launch_serves(run, 0, false) &&
                          (!auto_makeup_call || e->d_block_power != nullptr) && wins.size() >= 2;
  if (persistent) {
    AF_HIP(e->d_ready.reserve_exact(sizeof(int64_t)));
    AF_HIP(hipMemsetAsync(e->d_ready, 0, sizeof(int64_t), stream));
  }
  {  // the side streams start after whatever the caller queued before this call
    hipEvent_t ev;
    if (int rc = next_event(&ev)) return rc;
    AF_HIP(hipEventRecord(ev, stream));
    AF_HIP(hipStreamWaitEvent(e->aux_stream, ev, 0));
    AF_HIP(hipStreamWaitEvent(e->pre_stream, ev, 0));
    AF_HIP(hipStreamWaitEvent(e->ana_stream, ev, 0));
    if (syn != stream) AF_HIP(hipStreamWaitEvent(syn, ev, 0));
    if (fin && fin != stream) AF_HIP(hipStreamWaitEvent(fin, ev, 0));
    if (e->eq_stream != stream) AF_HIP(hipStreamWaitEvent(e->eq_stream, ev, 0));
    if (e->lim_stream) AF_HIP(hipStreamWaitEvent(e->lim_stream, ev, 0));
  }
  constexpr int kXh = af::SuppressorHost::kXhBuffers;
  // Pipeline depth.  The spectrum / record buffers of window w are free again when its synthesis has ended, and the synthesis
  // of w needs the analysis of w: with D buffer sets the loop analysis(w + D) <- synthesis(w) <- network(w) <- pitch spectra(w)
  // <- analysis(w) bounds the window period by (sum of those kernels) / D.  Round 2 ran D = 2 (the trace showed exactly that
  // period: 7.3 ms of dependent kernels per two windows); AF_SUPP_DEPTH=2 restores it for A/B runs.
  const int depth = sw.supp_depth;
  const int ana_ahead = depth - 1, pre_ahead = depth;  // windows the analysis / the pre-pass run ahead of the synthesis
  auto window_args = [&](int64_t index) {
    af::SuppArgs sa{};
    sa.in = src;
    sa.in_stride = src_stride;
    sa.out = out;
    e->supp.window_buffers(sa, index, depth, index > 0 ? wins[index - 1].nf : 0);
    sa.stream_stride = stream_stride;
    sa.n_streams = e->n_streams;
    sa.n_frames = (int)wins[index].nf;
    sa.frame0 = wins[index].f0;
    sa.strength = e->supp.strength;
    sa.smoothing_coeff = 1.0f - std::exp(-((480.0f / 48000.0f) / (15.0f / 1000.0f)));  // rnnoise.rs:45-51
    sa.raw_protocol = e->supp.raw_protocol ? 1 : 0;
    supp_front_end(e, run, front_flags, sa);
    if (e->gate_enabled) {
      sa.front_scrub = (front_flags || (e->base().params.flags & af::kFlagInputScrub)) ? 1 : 0;
      gate_args(e, sa);
    }
    return sa;
  };
  const int64_t n_windows = (int64_t)wins.size();
  std::vector<hipEvent_t> pre_done(n_windows), ana_done(n_windows), syn_done(n_windows);
  std::vector<hipEvent_t> rnn_done(n_windows);
  for (int64_t w = 0; w < n_windows; ++w) {
    if (int rc = next_event(&rnn_done[w])) return rc;
    if (int rc = next_event(&pre_done[w])) return rc;
    if (int rc = next_event(&ana_done[w])) return rc;
    if (int rc = next_event(&syn_done[w])) return rc;
  }
  // Stages are enqueued in pipeline order (the pre-pass two windows and the analysis one window ahead of the
  // synthesis), so that every event a stage waits on has been recorded before the wait is enqueued.
  auto enqueue_pre = [&](int64_t w) -> int {
    if (w >= kXh) AF_HIP(hipStreamWaitEvent(e->pre_stream, syn_done[w - kXh], 0));  // its model-input buffer is free
    if (fused_gate) {  // (a window holds whole control blocks: its first block is f0 x 480 / cb)
      af::VadGateArgs va = vad_args;
      va.block0 = wins[w].f0 * af::kRnnFrame / cb;
      AF_HIP(af::launch_vad_gate_pass(window_args(w), va, e->pre_stream));
      e->last_launches += 1;  // the control pass (the per-sample pass stands where the expander pre-pass is counted)
    } else {
      AF_HIP(af::launch_suppressor_prefilter(window_args(w), e->pre_stream));
    }
    AF_HIP(hipEventRecord(pre_done[w], e->pre_stream));
    e->supp.last_xh_slot = (int)(w % kXh);  // (af_suppressor_debug_read_model_input)
    e->supp.last_xh_frames = (int)wins[w].nf;
    return AF_OK;
  };
  auto enqueue_ana = [&](int64_t w) -> int {
    AF_HIP(hipStreamWaitEvent(e->ana_stream, pre_done[w], 0));
    if (w >= depth) AF_HIP(hipStreamWaitEvent(e->ana_stream, syn_done[w - depth], 0));  // its spectrum / record buffers are free
    // ORDERING THAT IS LOAD-BEARING: the pitch search of window w + 1 and the pitch tracker of window w must stay on this ONE
    // stream, in this order.  The whitened pitch buffers (`d_ds`, 3.4 KB per frame and stream) are a single set: the tracker of
    // window w reads what the search of window w wrote, and nothing but stream order keeps the search of w + 1 from overwriting
    // it first.  (Round 2 moved the tracker to the pre-pass stream to shorten this stream: run-to-run bit-identity was lost --
    // that race.  Moving either kernel needs a second `d_ds` set and an event from the tracker to the next search.)  The
    // tracker also owns the stream's pitch state rows (last period / gain, cepstral ring, the 1728-sample history a NEW call's
    // first pre-pass reads: ordered through the caller's stream at the end of the call).
    AF_HIP(af::launch_suppressor_analysis(window_args(w), e->supp.tables, e->ana_stream));
    AF_HIP(hipEventRecord(ana_done[w], e->ana_stream));
    return AF_OK;
  };
  // a window is behind us: crossfade bookkeeping may have moved the parameters on
  auto window_done = [&](int64_t seg_n) {
    run = e->base().params;
    if (strip_front) run.flags &= ~(front | af::kFlagInputScrub);
    blocks_done += (seg_n + cb - 1) / cb;
  };
  if (persistent) {  // the call's one chain launch: resident on the chain's CUs from here on, following `d_ready`
    af::ChainParams run_p = run;
    run_p.flags = (run_p.flags & ~af::kFlagEq) | af::kFlagInputDone;  // (what every window's launch was given)
    const int64_t total = frames * af::kRnnFrame;
    if (int rc = launch_chain_segment(e, run_p, run_modified, out, out, total, stream_stride, c.layout, e->samples_processed, e->d_stats,
                                      e->has_evidence ? e->d_vad : nullptr, e->aux_stream, stream, /*stats_cleared=*/true,
                                      auto_makeup_call ? e->d_block_power : nullptr, e->d_ready))
      return rc;
    eq_needs_chain_done = false;  // (an event behind THIS launch would make the first EQ wait for the launch that waits for it)
  }
  for (int64_t w = 0; w < std::min<int64_t>(pre_ahead, n_windows); ++w)
    if (int rc = enqueue_pre(w)) return rc;
  for (int64_t w = 0; w < std::min<int64_t>(ana_ahead, n_windows); ++w)
    if (int rc = enqueue_ana(w)) return rc;
  for (int64_t w = 0; w < n_windows; ++w) {
    const int64_t f0 = wins[w].f0, nf = wins[w].nf;
    AF_HIP(hipStreamWaitEvent(syn, ana_done[w], 0));
    if (fin && fin != syn && w >= depth) AF_HIP(hipStreamWaitEvent(syn, syn_done[w - depth], 0));  // its pitch-spectrum buffer is free
    AF_HIP(af::launch_suppressor_synthesis(window_args(w), e->supp.tables, e->supp.dw, syn, rnn_done[w], fin));
    if (e->trace) {  // the window's (silence, pitch index) decisions, before its record buffer is handed back to the analysis
      const af::SuppArgs sa = window_args(w);
      AF_HIP(hipMemcpy2DAsync(e->d_trace + 2 * f0 * e->n_streams, 2 * sizeof(int32_t),
                              reinterpret_cast<const char *>(sa.rec) + offsetof(af::SuppFrameRec, silence), sizeof(af::SuppFrameRec),
                              2 * sizeof(int32_t), (size_t)(nf * e->n_streams), hipMemcpyDeviceToDevice, last_supp));
    }
    AF_HIP(hipEventRecord(syn_done[w], last_supp));
    e->last_launches += 7;
    if (w + pre_ahead < n_windows)
      if (int rc = enqueue_pre(w + pre_ahead)) return rc;
    if (w + ana_ahead < n_windows)
      if (int rc = enqueue_ana(w + ana_ahead)) return rc;
    const int64_t seg0 = f0 * af::kRnnFrame, seg_n = nf * af::kRnnFrame;
    af::ChainParams run_w = run;
    bool eq_offloaded = false;
    double *power_w = nullptr;  // the window's block powers, when its systolic EQ launch was an auto-makeup pre-pass
    if (e->pipe.active && !sw.diag_skip_chain) {
      // ---- the window's chain as one more step of the stage pipeline (af_stages.hip; small and medium batches): this window
      // enters (its EQ stage reads the overlap-add output), the windows before it move one stage on
      const hipStream_t ds = e->pipe.stream;
      AF_HIP(hipStreamWaitEvent(ds, syn_done[w], 0));
      e->last_kernel_used = AF_KERNEL_STAGED;
      e->pipe.call_stride = stream_stride;
      int64_t sub_blocks = 0;
      for (int64_t off = 0; off < seg_n; off += chain_tw) {
        const int64_t n_sub = std::min<int64_t>(chain_tw, seg_n - off);
        af::DiagWin wd = diag_window(e, (int64_t)diag_wins.size(), seg0 + off, n_sub, blocks_done + sub_blocks, out + seg0 + off, out + seg0 + off);
        bool crossfade = false;
        if (int rc = stage_diag_eq_params(e, ds, &crossfade, &wd.eq_slot)) return rc;
        wd.eq_crossfade = crossfade ? 1 : 0;
        diag_wins.push_back(wd);
        if (int rc = stage_diag_step(e, run, diag_plan, diag_wins, (int64_t)diag_wins.size() - 1, ds)) return rc;
        advance_crossfades(e, n_sub);
        sub_blocks += (n_sub + cb - 1) / cb;
      }
      window_done(seg_n);
      continue;
    }
    // ---- the window's EQ on the suppressor's side (af_eq_systolic.hip), when the chain's launch would be the plain
    // one-launch form of the token-ring kernel
    if (eq_offload && !sw.diag_skip_chain) {
      const std::vector<af::ChainParams> runs_eq = run_params(e, e->base().params.flags & ~run.flags);  // (strip: what the pre-pass has taken over)
      bool ok = true, xf_w = false;
      for (const af::ChainParams &run_eq : runs_eq) {
        ok = ok && eq_side_launch_serves(run_eq, 0, false);
        // (a pending coefficient crossfade -- the 72 samples the legacy setters open a stream with -- runs in the systolic
        // kernel's general form; round 2 kept such windows' EQ inside the chain launch)
        xf_w = xf_w || eq_crossfade_pending(run_eq);
      }
      if (ok) {
        const hipStream_t es = e->eq_stream;  // behind the window's overlap-add, beside the next window's synthesis
        AF_HIP(hipStreamWaitEvent(es, syn_done[w], 0));
        // (always on the EQ stream, never the caller's: a copy on the legacy default stream waits for every other stream --
        // the resident chain launch included, which waits for this window: the call would run into the launch's bound)
        AF_HIP(e->d_params_eq.sync(runs_eq.data(), runs_eq.size(), e->stager, es));
        if (eq_needs_chain_done) {  // the previous window's EQ ran inside its chain launch: that launch owns the memories until it ends
          hipEvent_t chain_done;
          if (int rc = next_event(&chain_done)) return rc;
          AF_HIP(hipEventRecord(chain_done, e->aux_stream));
          AF_HIP(hipStreamWaitEvent(es, chain_done, 0));
          eq_needs_chain_done = false;
        }
        power_w = auto_makeup_call ? e->d_block_power + blocks_done * e->n_streams : nullptr;
        AF_HIP(af::launch_eq_systolic(e->d_params_eq, e->n_presets() == 1 ? nullptr : e->d_group_preset, e->d_st64, out + seg0, out + seg0, nullptr, nullptr, 0, 0,
                                      e->d_stats + blocks_done * e->n_streams, xf_w, seg_n, stream_stride, e->n_streams, es, power_w,
                                      // the lane-per-stream form where the suppressor's kernels want the issue slots and nothing waits
                                      // for the EQ's own latency (an auto-makeup window's block powers do): 184.5 -> 182.4 ms per step
                                      (e->n_presets() == 1 && (!power_w || sw.eq_stream_power) && (runs_eq[0].flags & af::kFlagEq)) ? runs_eq[0].n_eq_sections : -1));
        e->last_launches += 1;
        if (persistent) {  // the running chain launch picks the window up from here
          AF_HIP(af::launch_chain_publish_ready(e->d_ready, seg0 + seg_n, es));
          advance_crossfades(e, seg_n);  // (the one chain launch did not: the EQ's counters move window by window)
          window_done(seg_n);
          continue;
        }
        hipEvent_t eq_done;
        if (int rc = next_event(&eq_done)) return rc;
        AF_HIP(hipEventRecord(eq_done, es));
        AF_HIP(hipStreamWaitEvent(e->aux_stream, eq_done, 0));
        run_w.flags = (run_w.flags & ~af::kFlagEq) | af::kFlagInputDone;
        eq_offloaded = true;
      }
    }
    if (persistent) return fail(AF_ERR_BACKEND, "internal: a window of a one-launch call could not take the EQ on the suppressor's side");
    if (!eq_offloaded) {
      AF_HIP(hipStreamWaitEvent(e->aux_stream, syn_done[w], 0));
      eq_needs_chain_done = true;
    }
    if (!sw.diag_skip_chain)
      if (int rc = launch_chain_segment(e, run_w, run_modified, out + seg0, out + seg0, seg_n, stream_stride, c.layout,
                                        e->samples_processed + seg0, e->d_stats + blocks_done * e->n_streams,
                                        e->has_evidence ? e->d_vad + blocks_done * e->n_streams : nullptr, e->aux_stream, stream,
                                        /*stats_cleared=*/true, power_w))
        return rc;
    window_done(seg_n);
  }
  if (e->timing) AF_HIP(hipEventRecord(e->ev_mid.get(), last_supp));  // last suppressor kernel done
  if (syn != stream && n_windows > 0) AF_HIP(hipStreamWaitEvent(stream, syn_done[n_windows - 1], 0));
  {
    hipEvent_t ev;
    if (int rc = next_event(&ev)) return rc;
    AF_HIP(hipEventRecord(ev, e->aux_stream));
    AF_HIP(hipStreamWaitEvent(stream, ev, 0));
    if (e->lim_stream) {
      if (int rc = next_event(&ev)) return rc;
      AF_HIP(hipEventRecord(ev, e->lim_stream));
      AF_HIP(hipStreamWaitEvent(stream, ev, 0));
    }
  }
  if (e->pipe.active && !diag_wins.empty()) {
    const hipStream_t ds = e->pipe.stream;
    for (int64_t j = (int64_t)diag_wins.size(); j < (int64_t)diag_wins.size() + diag_plan.depth; ++j)  // the pipeline empties
      if (int rc = stage_diag_step(e, run, diag_plan, diag_wins, j, ds)) return rc;
    e->pipe.windows += (int64_t)diag_wins.size();
    hipEvent_t ev;
    if (int rc = next_event(&ev)) return rc;
    AF_HIP(hipEventRecord(ev, ds));
    AF_HIP(hipStreamWaitEvent(stream, ev, 0));
  }
  return AF_OK;
}

static int process_device_impl(af_engine *e, const float *in, float *out, int64_t n_samples, int64_t stream_stride, int32_t layout,
                               void *hip_stream) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (n_samples < 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_samples must be >= 0");
  if (layout != AF_LAYOUT_STREAM_MAJOR && layout != AF_LAYOUT_TIME_MAJOR)
    return fail(AF_ERR_INVALID_ARGUMENT, "unknown layout %d", layout);
  if (n_samples > 0 && (!in || !out)) return fail(AF_ERR_INVALID_ARGUMENT, "audio pointers are null");
  const int64_t min_stride = layout == AF_LAYOUT_STREAM_MAJOR ? n_samples : e->n_streams;
  if (stream_stride < min_stride) return fail(AF_ERR_INVALID_ARGUMENT, "stream_stride %lld is smaller than %lld",
                                              (long long)stream_stride, (long long)min_stride);
  if (int rc = ensure_started(e)) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  // ---- Everything that can refuse the call is checked before the engine's frame ring, its buffers or a stream are touched: a
  // refused call leaves af_engine_pending_input and the audio state as they were.
  // RNNoise frame buffering (rnnoise.rs:114-164: push_samples -> process_frames -> pop): the suppressor eats whole 480-sample
  // frames; what a call leaves over waits in the engine for the next call, and a call returns the whole frames that are
  // complete by then: floor((pending + n) / 480) * 480 samples per stream, which may be 0 or exceed n.
  const float *src = in;
  int64_t src_stride = stream_stride;
  const int64_t n_in = n_samples;
  int64_t n_run = n_samples, rem = 0;
  if (e->gate_enabled && layout != AF_LAYOUT_STREAM_MAJOR) return fail(AF_ERR_UNSUPPORTED, "the noise gate needs stream-major audio");
  if (e->supp.enabled) {
    if (layout != AF_LAYOUT_STREAM_MAJOR) return fail(AF_ERR_UNSUPPORTED, "the suppressor needs stream-major audio");
    const int64_t total = e->pending + n_in;
    n_run = (total / af::kRnnFrame) * af::kRnnFrame;
    rem = total - n_run;
    if (n_run > stream_stride)
      return fail(AF_ERR_INVALID_ARGUMENT, "this call completes %lld samples per stream (%d were pending): stream_stride %lld is too small",
                  (long long)n_run, e->pending, (long long)stream_stride);
  }
  const int cb = e->base().params.control_block;
  const int64_t blocks = (n_run + cb - 1) / cb;
  if (int rc = check_evidence_blocks(e, n_run)) return rc;
  if (n_run > 0 && !e->pipe.decided) {  // first call after a reset: which form of the chain this engine runs
    af::ChainParams probe = e->base().params;
    if (e->supp.enabled || e->gate_enabled) probe.flags &= ~(af::kFlagInputClamp | af::kFlagDcBlock | af::kFlagPreHighpass | af::kFlagInputScrub);
    const bool serves = stage_pipe_serves(e, probe, layout);
    const int env_staged = af::switches().staged;  // AF_STAGED=0 / 1: keep AUTO off / on the stage pipeline (A/B runs)
    if (e->kernel == AF_KERNEL_STAGED && !serves)
      return fail(AF_ERR_UNSUPPORTED, "the stage pipeline does not build this configuration (EQ-before-de-esser order, front end without the "
                                      "suppressor, more than 16 EQ sections, presets that differ in which stages run, time-major audio)");
    // (with the de-esser at any batch: its lane-per-stream form takes 417 ms per 2 s of audio whatever the batch)
    // (and several presets with auto-makeup: the token-ring kernel's pre-pass pair is a single-preset build)
    const bool deesser_staged = (probe.flags & af::kFlagDeesser) != 0 ||
                                (e->n_presets() > 1 && (probe.flags & af::kFlagCompressor) && probe.comp.auto_makeup_enabled);
    // (the per-stream lifecycle keeps AUTO off the pipeline, whose rings are the histories: the forms above its stream limit serve)
    e->pipe.active = serves && !e->life.enabled && (e->kernel == AF_KERNEL_STAGED || (e->kernel == AF_KERNEL_AUTO && env_staged != 0 &&
                                 (deesser_staged || e->n_streams <= (e->supp.enabled ? kStagedAutoMaxStreamsBehindSuppressor : kStagedAutoMaxStreams))) ||
                                (e->kernel == AF_KERNEL_AUTO && env_staged > 0));
    e->pipe.decided = true;
    if (e->pipe.active)
      if (int rc = stage_pipe_clear(e)) return rc;
  }
  if (front_end_in_gate_prepass(e) && layout != AF_LAYOUT_STREAM_MAJOR)
    return fail(AF_ERR_UNSUPPORTED, "this engine runs its front end in the noise gate's pre-pass, which needs stream-major audio");
  // ---- accepted: from here on the call only fails on a backend error
  if (e->gate_enabled && !e->d_gate) {
    AF_HIP(e->d_gate.reserve_exact(sizeof(int64_t) * af::kGateFields * e->n_streams));
    AF_HIP(e->d_gate.keep_if(hipMemset(e->d_gate, 0, sizeof(int64_t) * af::kGateFields * e->n_streams)));
  }
  e->last_stream = stream;
  e->retired.collect(false);
  const bool fused_gate = n_run > 0 && gate_vad_fused(e);
  af::VadGateArgs vad_args{};
  if (fused_gate)
    if (int rc = vad_gate_prepare(e, blocks, stream, vad_args)) return rc;
  if (e->supp.enabled) {
    const int64_t B = e->n_streams;
    if (e->pending > 0 || rem > 0) {
      AF_HIP(e->d_pending.reserve_exact(sizeof(float) * af::kRnnFrame * B));
      const size_t f4 = sizeof(float);
      if (n_run > 0) {
        AF_HIP(e->d_asm.reserve_retiring(f4 * B * n_run, e->retired, stream));  // (scratch of one call: grown geometrically, the old buffer retired)
        // [pending | head of this call] -> whole frames; the tail of this call waits (copied before anything writes `out`,
        // which may alias `in`)
        if (e->pending > 0)
          AF_HIP(hipMemcpy2DAsync(e->d_asm, f4 * n_run, e->d_pending, f4 * af::kRnnFrame, f4 * e->pending, B, hipMemcpyDeviceToDevice, stream));
        AF_HIP(hipMemcpy2DAsync(e->d_asm + e->pending, f4 * n_run, in, f4 * stream_stride, f4 * (n_run - e->pending), B,
                                hipMemcpyDeviceToDevice, stream));
        if (rem > 0)
          AF_HIP(hipMemcpy2DAsync(e->d_pending, f4 * af::kRnnFrame, in + (n_in - rem), f4 * stream_stride, f4 * rem, B,
                                  hipMemcpyDeviceToDevice, stream));
        src = e->d_asm;
        src_stride = n_run;
      } else if (n_in > 0) {
        AF_HIP(hipMemcpy2DAsync(e->d_pending + e->pending, f4 * af::kRnnFrame, in, f4 * stream_stride, f4 * n_in, B,
                                hipMemcpyDeviceToDevice, stream));
      }
      e->pending = (int)rem;
    }
    n_samples = n_run;
  }
  e->last_output_samples = n_samples;
  e->trace_frames = 0;
  e->ev_cursor = 0;
  e->last_blocks = blocks;
  e->last_kernel_ms = 0.0;
  e->last_launches = 0;
  if (n_samples == 0) return AF_OK;
  const int64_t rows = blocks * e->n_streams;
  AF_HIP(e->d_stats.reserve_retiring(sizeof(af::BlockStats) * rows, e->retired, stream));
  if (e->timing) {
    for (af::Event *ev : {&e->ev_start, &e->ev_stop, &e->ev_mid}) AF_HIP(ev->create());
    AF_HIP(hipEventRecord(e->ev_start.get(), stream));
  }
  e->chain_ms_events.clear();
  // live control: the state edits of the setters called since the last call that ran the chain (this call's first sample is
  // the chain's next one); the parameter blocks they changed are uploaded below like any other change
  if (int rc = launch_pending_retune(e, stream)) return rc;

  // ---- The noise gate without the suppressor: the front end and the gate run as the pre-pass (`in` -> `out`, on this stream),
  // and the chain then runs on `out` in place with the front end's flags stripped, as it does behind the suppressor.
  const uint32_t gate_strip = front_end_in_gate_prepass(e)
                                  ? (af::kFlagInputScrub | af::kFlagInputClamp | af::kFlagDcBlock | af::kFlagPreHighpass) : 0u;
  const float *chain_in = in;
  if (gate_strip) {
    const af::ChainParams &hp = e->base().params;
    af::SuppArgs sa{};
    sa.in = in;
    sa.in_stride = stream_stride;
    sa.out = out;
    sa.stream_stride = stream_stride;
    sa.n_streams = e->n_streams;
    sa.n_samples = n_samples;
    sa.front_scrub = (hp.flags & af::kFlagInputScrub) ? 1 : 0;
    supp_front_end(e, hp, hp.flags, sa);
    if (e->gate_enabled) gate_args(e, sa);  // (else the pass runs the front end alone and leaves the gate's state alone)
    if (fused_gate) {  // modes 1 / 2 with the controller attached: control pass + fused per-sample pass
      AF_HIP(af::launch_vad_gate_pass(sa, vad_args, stream));
      e->last_launches += 1;
    } else {
      AF_HIP(af::launch_gate_prepass(sa, stream));
    }
    e->last_launches += 1;
    if (e->timing) AF_HIP(hipEventRecord(e->ev_mid.get(), stream));  // the pre-pass counts as suppressor-side time
    chain_in = out;
  }
  const CallArgs call{chain_in, out, n_samples, stream_stride, layout, stream, gate_strip, rows};
  int rc;
  if (e->supp.enabled) rc = run_suppressor_pipeline(e, call, src, src_stride, fused_gate, vad_args);
  else if (e->pipe.active) rc = run_stage_pipeline(e, call);
  else rc = run_chain_launch(e, call);
  if (rc) return rc;
  if (e->timing) {  // ev_mid: suppressor-side time ends (the suppressor's path and the gate's pre-pass have recorded theirs)
    if (!e->supp.enabled && !gate_strip) AF_HIP(hipEventRecord(e->ev_mid.get(), stream));
    AF_HIP(hipEventRecord(e->ev_stop.get(), stream));
  }
  e->samples_processed += n_samples;
  return AF_OK;
}

int af_engine_process_device(af_engine *e, const float *in, float *out, int64_t n_samples, int64_t stream_stride,
                             int32_t layout, void *hip_stream) {
  if (e && io_resampled(e)) return fail(AF_ERR_UNSUPPORTED, "%s", kStreamOnlyMessage);
  if (e && e->mix) return fail(AF_ERR_UNSUPPORTED, "%s", kChannelsStreamOnlyMessage);
  if (e && e->ow) return fail(AF_ERR_UNSUPPORTED, "%s", kWriterStreamOnlyMessage);
  return process_device_impl(e, in, out, n_samples, stream_stride, layout, hip_stream);
}

// host buffers in, host buffers out: `in` is [streams][n_in] (stream-major) or [n_in][streams] (time-major), `out` gets
// *n_out samples per stream at out_stride (stream-major) -- n_out differs from n_in only with the suppressor on
static int process_host_impl(af_engine *e, const float *in, int64_t n_in, float *out, int64_t out_stride, int32_t layout,
                             int64_t *n_out) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (n_in < 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_samples must be >= 0");
  if (n_in > 0 && (!in || !out)) return fail(AF_ERR_INVALID_ARGUMENT, "audio pointers are null");
  if (int rc = ensure_started(e)) return rc;
  const int64_t B = e->n_streams;
  const bool stream_major = layout == AF_LAYOUT_STREAM_MAJOR;
  int64_t produced = n_in;
  if (e->supp.enabled) produced = ((e->pending + n_in) / af::kRnnFrame) * af::kRnnFrame;
  if (produced > 0 && !out) return fail(AF_ERR_INVALID_ARGUMENT, "audio pointers are null");
  if (stream_major && out_stride < produced)
    return fail(AF_ERR_INVALID_ARGUMENT, "this call completes %lld samples per stream (%d were pending) but `out` holds %lld: "
                "use af_engine_stream_host with a larger out_stride", (long long)produced, e->pending, (long long)out_stride);
  const int64_t io_stride = stream_major ? std::max<int64_t>(std::max(n_in, produced), 1) : B;
  const int64_t total = stream_major ? io_stride * B : n_in * B;
  AF_HIP(e->d_io.reserve_exact(sizeof(float) * total));
  if (n_in > 0) {
    if (stream_major)
      AF_HIP(hipMemcpy2D(e->d_io, sizeof(float) * io_stride, in, sizeof(float) * n_in, sizeof(float) * n_in, B, hipMemcpyHostToDevice));
    else
      AF_HIP(hipMemcpy(e->d_io, in, sizeof(float) * total, hipMemcpyHostToDevice));
  }
  if (int rc = process_device_impl(e, e->d_io, e->d_io, n_in, io_stride, layout, nullptr)) return rc;
  AF_HIP(hipStreamSynchronize(nullptr));
  if (produced > 0) {
    if (stream_major)
      AF_HIP(hipMemcpy2D(out, sizeof(float) * out_stride, e->d_io, sizeof(float) * io_stride, sizeof(float) * produced, B, hipMemcpyDeviceToHost));
    else
      AF_HIP(hipMemcpy(out, e->d_io, sizeof(float) * total, hipMemcpyDeviceToHost));
  }
  if (n_out) *n_out = produced;
  return check_device_status(e);
}

// the engine's output writer at the rate its output side runs at, with the limits dsp_loop.rs:781-795 derives from it
static int engine_build_writer(af_engine *e) {
  const double r = e->io_output_rate ? (double)e->io_output_rate : e->sample_rate;
  if (r != std::floor(r) || r <= 0 || r > INT32_MAX)
    return fail(AF_ERR_INVALID_ARGUMENT, "the output writer needs an integer output sample rate");
  const int32_t rate = (int32_t)r;
  af_output_writer_config cfg;
  if (int rc = af_output_writer_default_config(rate, &cfg)) return rc;
  af_output_writer *w = nullptr;
  if (int rc = af_output_writer_create(&cfg, e->n_streams, e->device, &w)) return rc;
  af_output_writer_destroy(e->ow);
  e->ow = w;
  e->ow_target_center = cfg.target_center;
  e->ow_capacity = cfg.queue_capacity;
  e->ow_fill.clear();
  e->ow_fill_dirty = true;
  e->ow_written.assign((size_t)e->n_streams, 0);
  return AF_OK;
}

// ---- device-rate I/O: dsp_loop.rs:274-317 (the two resamplers), 963-1011 (input side), 843-895 (output side)
int af_engine_set_io_sample_rates(af_engine *e, uint32_t input_rate, uint32_t output_rate) {
  if (int rc = require_config(e)) return rc;
  const uint32_t fs = (uint32_t)e->sample_rate;
  const bool want_in = input_rate != 0 && (double)input_rate != e->sample_rate;    // dsp_loop.rs:274
  const bool want_out = output_rate != 0 && (double)output_rate != e->sample_rate;  // dsp_loop.rs:292
  if ((want_in || want_out) && (double)fs != e->sample_rate)
    return fail(AF_ERR_INVALID_ARGUMENT, "the I/O resamplers need an integer engine sample rate");
  // build_sinc_resampler (resampling.rs:140-156): the product configuration, chunks of 1024
  af_stream_resampler *rin = nullptr, *rout = nullptr;
  if (want_in)
    if (int rc = af_stream_resampler_create(input_rate, fs, 1024, 128, AF_WINDOW_BLACKMAN, e->n_streams, e->device, &rin)) return rc;
  if (want_out)
    if (int rc = af_stream_resampler_create(fs, output_rate, 1024, 128, AF_WINDOW_BLACKMAN, e->n_streams, e->device, &rout)) {
      af_stream_resampler_destroy(rin);
      return rc;
    }
  af_stream_resampler_destroy(e->rs_in);
  af_stream_resampler_destroy(e->rs_out);
  e->rs_in = rin;
  e->rs_out = rout;
  e->io_output_rate = want_out ? output_rate : 0;
  if (e->ow) return engine_build_writer(e);  // the writer runs at the output side's rate
  return AF_OK;
}

int af_engine_io_resampler_delay(const af_engine *e, int32_t *input_frames, int32_t *output_frames) {  // dsp_loop.rs:310-313
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (input_frames) *input_frames = af_stream_resampler_output_delay(e->rs_in);
  if (output_frames) *output_frames = af_stream_resampler_output_delay(e->rs_out);
  return AF_OK;
}

int af_engine_io_resampler_pending(const af_engine *e, int64_t *input_frames, int64_t *output_frames) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (input_frames) *input_frames = af_stream_resampler_pending_input(e->rs_in);
  if (output_frames) *output_frames = af_stream_resampler_pending_input(e->rs_out);
  return AF_OK;
}

// ---- multichannel input: the capture callback's mixdown (input.rs:785-843) in front of the input resampler / the chain
int af_engine_set_input_channels(af_engine *e, int32_t n_channels, int32_t mode) {
  if (int rc = require_config(e)) return rc;
  af_mixdown *m = nullptr;
  if (int rc = af_mixdown_create(n_channels, mode, e->n_streams, e->device, &m)) return rc;
  af_mixdown_destroy(e->mix);
  e->mix = nullptr;
  if (n_channels > 1) e->mix = m;  // one channel: the feature is off, every call is as without this setter
  else af_mixdown_destroy(m);
  return AF_OK;
}

int af_engine_set_input_channel_mode(af_engine *e, int32_t mode) {  // live: the callback loads the mode per chunk (input.rs:814-816)
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (!e->mix) {
    if (mode < 0 || mode > 4) return fail(AF_ERR_INVALID_ARGUMENT, "unknown input channel mode %d", mode);
    return AF_OK;  // mono input: nothing to mix
  }
  return af_mixdown_set_mode(e->mix, mode);
}

int af_engine_read_input_phase(af_engine *e, float *stereo_correlation, uint64_t *phase_warning_count, int32_t *strategy,
                               float *estimated_delay, int32_t *polarity_flipped, int32_t n_streams) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (n_streams != e->n_streams) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be the engine's %d", e->n_streams);
  if (e->mix) return af_mixdown_read_diagnostics(e->mix, stereo_correlation, phase_warning_count, strategy, estimated_delay, polarity_flipped, n_streams);
  for (int32_t s = 0; s < n_streams; ++s) {  // mono input, input.rs:789-793: none / 0 / false, no correlation
    if (stereo_correlation) stereo_correlation[s] = std::numeric_limits<float>::quiet_NaN();
    if (phase_warning_count) phase_warning_count[s] = 0;
    if (strategy) strategy[s] = 0;
    if (estimated_delay) estimated_delay[s] = 0.0f;
    if (polarity_flipped) polarity_flipped[s] = 0;
  }
  return AF_OK;
}

// ---- the output writer behind the chain / the output resampler (output_writer.rs:62-343)
int af_engine_set_output_writer(af_engine *e, int32_t enabled) {
  if (int rc = require_config(e)) return rc;
  if (!enabled) {  // off: every call takes the branch it took before
    af_output_writer_destroy(e->ow);
    e->ow = nullptr;
    e->ow_fill.clear();
    e->ow_fill_dirty = true;
    e->ow_written.clear();
    return AF_OK;
  }
  return engine_build_writer(e);
}

int af_engine_set_output_queue_fill(af_engine *e, const int64_t *fill, int32_t n_streams) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (!e->ow) return fail(AF_ERR_STATE, "the output writer is off (af_engine_set_output_writer)");
  if (n_streams != e->n_streams) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be the engine's %d", e->n_streams);
  if (!fill) return fail(AF_ERR_INVALID_ARGUMENT, "fill is null");
  for (int32_t s = 0; s < n_streams; ++s)
    if (fill[s] < 0 || fill[s] > e->ow_capacity)
      return fail(AF_ERR_INVALID_ARGUMENT, "fill[%d] = %lld is outside the queue's 0 .. %lld", s, (long long)fill[s], (long long)e->ow_capacity);
  e->ow_fill.assign(fill, fill + n_streams);
  e->ow_fill_dirty = true;
  return AF_OK;
}

int af_engine_read_output_written(af_engine *e, int64_t *written, int32_t n_streams) {
  if (!e || !written) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (!e->ow) return fail(AF_ERR_STATE, "the output writer is off (af_engine_set_output_writer)");
  if (n_streams != e->n_streams) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be the engine's %d", e->n_streams);
  for (int32_t s = 0; s < n_streams; ++s) written[s] = e->ow_written[(size_t)s];
  return AF_OK;
}

int af_engine_read_output_counters(af_engine *e, uint64_t *jitter_dropped, uint64_t *retime_adjustments, uint64_t *recovery_events,
                                   uint64_t *short_write_dropped, uint64_t *clip_events, uint64_t *true_peak_events, int32_t n_streams) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (!e->ow) return fail(AF_ERR_STATE, "the output writer is off (af_engine_set_output_writer)");
  return af_output_writer_read_counters(e->ow, jitter_dropped, retime_adjustments, recovery_events, short_write_dropped, clip_events,
                                        true_peak_events, n_streams);
}

int af_engine_read_output_meters(af_engine *e, float *db, float *linear, float *ratio, float *drift_ema, int64_t *out_len,
                                 int64_t *fade_remaining, int64_t *fill_after, int32_t n_streams) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (!e->ow) return fail(AF_ERR_STATE, "the output writer is off (af_engine_set_output_writer)");
  return af_output_writer_read_meters(e->ow, db, linear, ratio, drift_ema, out_len, fade_remaining, fill_after, n_streams);
}

// host arithmetic only: what the next af_engine_stream_host call of n_in frames will do (m3: frames into the output writer)
static int stream_frames(const af_engine *e, int64_t n_in, int64_t *engine_frames_in, int64_t *engine_frames_out, int64_t *n_out);
int af_engine_stream_plan(const af_engine *e, int64_t n_in, int64_t *engine_frames_in, int64_t *engine_frames_out, int64_t *n_out) {
  int64_t m3 = 0;
  if (int rc = stream_frames(e, n_in, engine_frames_in, engine_frames_out, &m3)) return rc;
  if (e->ow && m3 > 0) m3 = af_output_writer_max_output_frames(e->ow, m3);  // the longest row the writer can yield
  if (n_out) *n_out = m3;
  return AF_OK;
}
static int stream_frames(const af_engine *e, int64_t n_in, int64_t *engine_frames_in, int64_t *engine_frames_out, int64_t *n_out) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (n_in < 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_samples must be >= 0");
  const int64_t m1 = e->rs_in ? af_stream_resampler_output_frames(e->rs_in, n_in) : n_in;
  int64_t m2 = m1;
  if (e->supp.enabled) m2 = (e->rs_in && m1 == 0) ? 0 : ((e->pending + m1) / af::kRnnFrame) * af::kRnnFrame;  // (no chunk: no engine call)
  const int64_t m3 = e->rs_out ? (m2 > 0 ? af_stream_resampler_output_frames(e->rs_out, m2) : 0) : m2;
  if (engine_frames_in) *engine_frames_in = m1;
  if (engine_frames_out) *engine_frames_out = m2;
  if (n_out) *n_out = m3;
  return AF_OK;
}

// af_engine_stream_host with a rate set: input resampler -> the engine's device path on an internal buffer -> output
// resampler, all on the null stream.  Everything that can refuse the call is checked before either resampler or the engine is
// touched.  DEVIATION: non-finite host input refuses the call.  The reference resamples first and scrubs afterwards
// (dsp_loop.rs:963-1011, then routing.rs:802-823), which smears one NaN over the 2 * sinc_len frames whose windows hold it
// before zeroing them all; here the padded sinc rows would spread it further (a NaN times a zero pad tap is a NaN).
static int stream_host_resampled(af_engine *e, const float *in, int64_t n_in, float *out, int64_t out_stride, int64_t *n_out) {
  if (n_in < 0) return fail(AF_ERR_INVALID_ARGUMENT, "n_samples must be >= 0");
  if (n_in > 0 && !in) return fail(AF_ERR_INVALID_ARGUMENT, "audio pointers are null");
  int64_t m1 = 0, m2 = 0, m3 = 0;
  if (int rc = stream_frames(e, n_in, &m1, &m2, &m3)) return rc;
  if (m3 > 0 && !out) return fail(AF_ERR_INVALID_ARGUMENT, "audio pointers are null");
  if (e->ow && m3 > af::kOwMaxBlock)
    return fail(AF_ERR_INVALID_ARGUMENT, "this call hands the output writer %lld frames per stream; it takes at most %d",
                (long long)m3, af::kOwMaxBlock);
  const int64_t ow_width = (e->ow && m3 > 0) ? af_output_writer_max_output_frames(e->ow, m3) : 0;
  if (out_stride < std::max(m3, ow_width))
    return fail(AF_ERR_INVALID_ARGUMENT, "this call produces %lld frames per stream (af_engine_stream_plan) but out_stride is %lld",
                (long long)std::max(m3, ow_width), (long long)out_stride);
  const int64_t B = e->n_streams;
  const int64_t C = e->mix ? af_mixdown_channels(e->mix) : 1;  // in[(s * n_in + t) * C + c]
  if (!af::check_finite(in, 1, B * n_in * C, 0)) return fail(AF_ERR_NON_FINITE, "samples must be finite");
  if (int rc = ensure_started(e)) return rc;
  if (int rc = check_evidence_blocks(e, m2)) return rc;
  // ---- accepted
  const int64_t f4 = sizeof(float);
  const int64_t mid_stride = std::max<int64_t>(m1, 1) + af::kRnnFrame;  // the engine may return up to 479 frames more than it got
  AF_HIP(e->d_rs_in.reserve_retiring(f4 * B * std::max<int64_t>(n_in, 1), e->retired, nullptr));
  AF_HIP(e->d_rs_mid.reserve_retiring(f4 * B * mid_stride, e->retired, nullptr));
  AF_HIP(e->d_rs_out.reserve_retiring(f4 * B * std::max<int64_t>(m3, 1), e->retired, nullptr));
  int64_t got = 0;
  if (e->mix) {  // the capture callback's mixdown first (input.rs:785-843): mono into what the mono path would have uploaded
    AF_HIP(e->d_mix_in.reserve_retiring(f4 * B * C * std::max<int64_t>(n_in, 1), e->retired, nullptr));
    if (n_in > 0) {
      AF_HIP(hipMemcpy(e->d_mix_in, in, f4 * B * n_in * C, hipMemcpyHostToDevice));
      if (int rc = af_mixdown_push_device(e->mix, e->d_mix_in, n_in, n_in, e->rs_in ? e->d_rs_in : e->d_rs_mid,
                                          e->rs_in ? n_in : mid_stride, nullptr)) return rc;
    }
    if (e->rs_in)
      if (int rc = af_stream_resampler_push_device(e->rs_in, e->d_rs_in, n_in, std::max<int64_t>(n_in, 1), e->d_rs_mid, m1, mid_stride, &got, nullptr)) return rc;
  } else if (e->rs_in) {
    if (n_in > 0) AF_HIP(hipMemcpy(e->d_rs_in, in, f4 * B * n_in, hipMemcpyHostToDevice));
    if (int rc = af_stream_resampler_push_device(e->rs_in, e->d_rs_in, n_in, std::max<int64_t>(n_in, 1), e->d_rs_mid, m1, mid_stride, &got, nullptr)) return rc;
  } else if (n_in > 0) {
    AF_HIP(hipMemcpy2D(e->d_rs_mid, f4 * mid_stride, in, f4 * n_in, f4 * n_in, B, hipMemcpyHostToDevice));
  }
  if (m1 > 0) {  // (no chunk completed: the engine is not called, dsp_loop.rs:1013)
    if (int rc = process_device_impl(e, e->d_rs_mid, e->d_rs_mid, m1, mid_stride, AF_LAYOUT_STREAM_MAJOR, nullptr)) return rc;
  } else {
    e->last_output_samples = 0;
    e->last_blocks = 0;
  }
  const float *res = e->d_rs_mid;
  int64_t res_stride = mid_stride;
  if (e->rs_out && m2 > 0) {
    if (int rc = af_stream_resampler_push_device(e->rs_out, e->d_rs_mid, m2, mid_stride, e->d_rs_out, m3, std::max<int64_t>(m3, 1), &got, nullptr)) return rc;
    res = e->d_rs_out;
    res_stride = std::max<int64_t>(m3, 1);
  }
  if (e->ow) {  // write_chunk on what the chain / the output resampler produced (dsp_loop.rs:843-895)
    std::fill(e->ow_written.begin(), e->ow_written.end(), 0);
    if (m3 == 0) {  // nothing to write: the reference's write_chunk returns false on an empty block
      AF_HIP(hipStreamSynchronize(nullptr));
      return check_device_status(e);
    }
    AF_HIP(e->d_ow_fill.reserve_exact(sizeof(int64_t) * (size_t)B));
    AF_HIP(e->d_ow_written.reserve_exact(sizeof(int64_t) * (size_t)B));
    AF_HIP(e->d_ow_out.reserve_retiring(f4 * B * ow_width, e->retired, nullptr));
    if (e->ow_fill_dirty) {  // uploaded when af_engine_set_output_queue_fill (or a reset) changed it, not per call
      if (e->ow_fill.empty()) e->ow_fill.assign((size_t)B, e->ow_target_center);  // no evidence yet: no error
      AF_HIP(hipMemcpy(e->d_ow_fill, e->ow_fill.data(), sizeof(int64_t) * (size_t)B, hipMemcpyHostToDevice));
      e->ow_fill_dirty = false;
    }
    // limiter_enabled and the ceiling as the loop takes them from the limiter (dsp_loop.rs:535, output_writer.rs:208-215)
    if (int rc = af_output_writer_set_limiter(e->ow, e->base().proto.limiter_enabled ? 1 : 0,
                                              std::pow(10.0f, (float)e->base().proto.limiter.ceiling_db / 20.0f))) return rc;
    if (int rc = af_output_writer_push_device(e->ow, res, m3, res_stride, e->d_ow_fill, 0, e->d_ow_out, ow_width, ow_width,
                                              e->d_ow_written, nullptr)) return rc;
    AF_HIP(hipStreamSynchronize(nullptr));
    AF_HIP(hipMemcpy(e->ow_written.data(), e->d_ow_written, sizeof(int64_t) * (size_t)B, hipMemcpyDeviceToHost));
    int64_t longest = 0;
    for (int64_t v : e->ow_written) longest = std::max(longest, v);
    if (longest > 0) {
      AF_HIP(hipMemcpy2D(out, f4 * out_stride, e->d_ow_out, f4 * ow_width, f4 * longest, B, hipMemcpyDeviceToHost));
      for (int64_t s = 0; s < B; ++s)  // rows are zero beyond their own length
        std::fill(out + s * out_stride + e->ow_written[(size_t)s], out + s * out_stride + longest, 0.0f);
    }
    if (n_out) *n_out = longest;
    return check_device_status(e);
  }
  AF_HIP(hipStreamSynchronize(nullptr));
  if (m3 > 0) AF_HIP(hipMemcpy2D(out, f4 * out_stride, res, f4 * res_stride, f4 * m3, B, hipMemcpyDeviceToHost));
  if (n_out) *n_out = m3;
  return check_device_status(e);
}

int af_engine_process_host(af_engine *e, const float *in, float *out, int64_t n_samples, int32_t layout) {
  if (layout != AF_LAYOUT_STREAM_MAJOR && layout != AF_LAYOUT_TIME_MAJOR)
    return fail(AF_ERR_INVALID_ARGUMENT, "unknown layout %d", layout);
  if (e && io_resampled(e)) return fail(AF_ERR_UNSUPPORTED, "%s", kStreamOnlyMessage);
  if (e && e->mix) return fail(AF_ERR_UNSUPPORTED, "%s", kChannelsStreamOnlyMessage);
  if (e && e->ow) return fail(AF_ERR_UNSUPPORTED, "%s", kWriterStreamOnlyMessage);
  return process_host_impl(e, in, n_samples, out, layout == AF_LAYOUT_STREAM_MAJOR ? n_samples : (e ? e->n_streams : 0), layout, nullptr);
}

int af_engine_stream_host(af_engine *e, const float *in, int64_t n_in, float *out, int64_t out_stride, int64_t *n_out) {
  if (n_out) *n_out = 0;
  if (e && (io_resampled(e) || e->mix || e->ow)) return stream_host_resampled(e, in, n_in, out, out_stride, n_out);
  return process_host_impl(e, in, n_in, out, out_stride, AF_LAYOUT_STREAM_MAJOR, n_out);
}

int64_t af_engine_pending_input(const af_engine *e) { return e ? e->pending : 0; }
int64_t af_engine_last_output_samples(const af_engine *e) { return e ? e->last_output_samples : 0; }

// test tap: RNNoiseProcessor::scale_sample_for_model (rnnoise.rs:89-111) as the pre-pass kernel evaluates it
int af_suppressor_debug_scale_for_model(const float *in, float *out, int64_t n, int32_t device) {
  if ((!in || !out) && n > 0) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (n <= 0) return AF_OK;
  AF_HIP(hipSetDevice(device));
  af::DeviceBuffer<float> d;
  AF_HIP(d.reserve_exact(sizeof(float) * n));
  hipError_t err = hipMemcpy(d, in, sizeof(float) * n, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = af::launch_scale_probe(d, d, n, nullptr);
  if (err == hipSuccess) err = hipMemcpy(out, d, sizeof(float) * n, hipMemcpyDeviceToHost);
  if (err != hipSuccess) return fail(AF_ERR_BACKEND, "scale probe failed: %s", hipGetErrorString(err));
  return AF_OK;
}

int af_suppressor_set_trace_enabled(af_engine *e, int32_t on) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  e->trace = on != 0;
  return AF_OK;
}
int64_t af_suppressor_trace_frames(const af_engine *e) { return e ? e->trace_frames : 0; }
int af_suppressor_read_trace(af_engine *e, int32_t *out, int64_t capacity_frames) {
  if (!e || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (capacity_frames < e->trace_frames)
    return fail(AF_ERR_INVALID_ARGUMENT, "capacity %lld < %lld frames", (long long)capacity_frames, (long long)e->trace_frames);
  if (e->trace_frames == 0) return AF_OK;
  AF_HIP(e->use_device());
  AF_HIP(hipStreamSynchronize(e->last_stream));
  AF_HIP(hipMemcpy(out, e->d_trace, sizeof(int32_t) * 2 * e->trace_frames * e->n_streams, hipMemcpyDeviceToHost));
  return AF_OK;
}

int af_engine_synchronize(af_engine *e) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (!e->started) return AF_OK;
  AF_HIP(e->use_device());
  AF_HIP(hipStreamSynchronize(e->last_stream));
  return check_device_status(e);
}

int64_t af_engine_last_block_count(const af_engine *e) { return e ? e->last_blocks : 0; }
int64_t af_engine_samples_processed(const af_engine *e) { return e ? e->samples_processed : 0; }

int af_engine_read_block_stats(af_engine *e, af_block_stats *out, int64_t capacity) {
  if (!e || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  const int64_t rows = e->last_blocks * e->n_streams;
  if (capacity < rows) return fail(AF_ERR_INVALID_ARGUMENT, "capacity %lld < %lld rows", (long long)capacity, (long long)rows);
  if (rows == 0) return AF_OK;
  AF_HIP(e->use_device());
  AF_HIP(hipStreamSynchronize(e->last_stream));
  AF_HIP(hipMemcpy(out, e->d_stats, sizeof(af::BlockStats) * rows, hipMemcpyDeviceToHost));
  return check_device_status(e);
}

int af_engine_last_kernel_ms(af_engine *e, double *ms, int32_t *launches) {
  if (!e || !ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  *ms = 0.0;
  if (launches) *launches = e->last_launches;
  if (!e->timing || !e->ev_start || e->last_launches == 0) return AF_OK;
  AF_HIP(e->use_device());
  AF_HIP(hipEventSynchronize(e->ev_stop.get()));
  float t = 0.0f;
  AF_HIP(hipEventElapsedTime(&t, e->ev_start.get(), e->ev_stop.get()));
  *ms = (double)t;
  return AF_OK;
}

int af_engine_last_stage_ms(af_engine *e, double *suppressor_ms, double *chain_ms) {
  if (!e || !suppressor_ms || !chain_ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  *suppressor_ms = *chain_ms = 0.0;
  if (!e->timing || !e->ev_start || e->last_launches == 0) return AF_OK;
  AF_HIP(e->use_device());
  AF_HIP(hipEventSynchronize(e->ev_stop.get()));
  float t = 0.0f;
  AF_HIP(hipEventElapsedTime(&t, e->ev_start.get(), e->ev_mid.get()));
  *suppressor_ms = (double)t;
  for (const af::TimedSpan &span : e->chain_ms_events) {
    double ms = 0.0;
    AF_HIP(span.elapsed_ms(&ms));
    *chain_ms += ms;  // summed over the chain launches of the call (they may overlap suppressor kernels)
  }
  return AF_OK;
}

int af_engine_last_chain_launch_ms(af_engine *e, double *first_ms, double *tail_ms, int32_t *segments) {
  if (!e || !first_ms || !tail_ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  *first_ms = *tail_ms = 0.0;
  if (segments) *segments = (int32_t)e->chain_ms_events.size();
  if (!e->timing || !e->ev_start || e->last_launches == 0) return AF_OK;
  AF_HIP(e->use_device());
  for (const af::TimedSpan &span : e->chain_ms_events) {
    double ms = 0.0;
    AF_HIP(span.elapsed_ms(&ms));
    *first_ms += ms;
  }
  return AF_OK;
}

// ---- per-stream lifecycle: restart, export and import of single streams between calls (af_stream_state.h) ----------------
int af_engine_set_stream_lifecycle(af_engine *e, int32_t enabled) {
  if (int rc = require_config(e)) return rc;
  e->life.enabled = enabled != 0;
  return AF_OK;
}

namespace {
namespace ss = af::sstate;

// the shape record of a slot of preset k.  Before streaming started (af_engine_stream_state_size) the planes' heights are
// what the first call would allocate, and the gate plane exists if the gate is on.
ss::Shape lifecycle_shape(af_engine *e, int k) {
  int n64 = e->n_f64, n32 = e->n_f32, first_live = 0;
  if (!e->started) {
    export_params(e);
    plane_heights(e, &n64, &n32, &first_live);
  }
  const af::ChainParams &hp = e->presets[k].params;
  ss::Shape s{};
  s.sample_rate = e->sample_rate;
  s.control_block = hp.control_block;
  s.n_eq_sections = hp.n_eq_sections;
  s.lookahead = e->presets[k].proto.limiter.lookahead_samples;
  s.meter_slots = preset_meter_slots(e, k);
  s.stage_flags = (hp.flags & ss::kStageMask) | (s.meter_slots > 0 ? ss::kStageAutoMakeup : 0u);
  s.suppressor = e->supp.enabled ? 1 : 0;
  s.gate_plane = (e->d_gate || (!e->started && e->gate_enabled)) ? 1 : 0;
  s.live_rows = e->live_control ? 1 : 0;
  s.rows64 = n64;
  s.rows32 = af::kF32Fixed + (n32 - af::kF32Fixed) / 2;
  return s;
}

// Everything that refuses a lifecycle call, in two halves: the arguments and what the engine's configuration rules out
// (decided in configuration mode too); then not started, and what the engine's momentary state rules out.  An import checks
// its blobs' headers between the two.  None of it needs the device, and a refused call has touched nothing.
int lifecycle_accepts_config(af_engine *e, const char *what, const int32_t *streams, int32_t n) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (!e->life.enabled)
    return fail(AF_ERR_STATE, "%s needs af_engine_set_stream_lifecycle(e, 1), a configuration setter (off by default)", what);
  const std::string msg = ss::check_list(streams, n, e->n_streams);
  if (!msg.empty()) return fail(AF_ERR_INVALID_ARGUMENT, "%s: %s", what, msg.c_str());
  // objects that keep per-stream state of their own, which a blob does not carry and a restart would not reach
  if (e->rs_in || e->rs_out)
    return fail(AF_ERR_UNSUPPORTED, "%s: device-rate I/O is set (af_engine_set_io_sample_rates); the resamplers keep per-stream "
                                    "histories the stream lifecycle does not cover", what);
  if (e->mix)
    return fail(AF_ERR_UNSUPPORTED, "%s: multichannel input is set (af_engine_set_input_channels); the mixdown keeps per-stream "
                                    "state the stream lifecycle does not cover", what);
  if (e->ow)
    return fail(AF_ERR_UNSUPPORTED, "%s: the output writer is set (af_engine_set_output_writer); it keeps per-stream state the "
                                    "stream lifecycle does not cover", what);
  if (e->gate_vad_attached)
    return fail(AF_ERR_UNSUPPORTED, "%s: the VAD-fused gate is attached (af_gate_set_vad_auto_gate_enabled); its controller plane "
                                    "is not part of a stream's state blob", what);
  if (e->kernel == AF_KERNEL_STAGED)
    return fail(AF_ERR_UNSUPPORTED, "%s: the stage pipeline is selected; its hand-over rings hold the streams' histories", what);
  return AF_OK;
}
int lifecycle_accepts_state(af_engine *e, const char *what) {
  if (!e->started) return fail(AF_ERR_STATE, "%s: streaming has not started; a stream's lifecycle begins with the first process call", what);
  if (e->pipe.active) return fail(AF_ERR_UNSUPPORTED, "%s: the stage pipeline is active; its hand-over rings hold the streams' histories", what);
  if (e->pending > 0)
    return fail(AF_ERR_UNSUPPORTED, "%s: %d samples per stream are pending in the suppressor's frame assembly, which all streams share; "
                                    "feed whole 480-sample frames first", what, e->pending);
  const int cb = e->base().params.control_block;
  if (cb > 0 && e->samples_processed % cb != 0)
    return fail(AF_ERR_UNSUPPORTED, "%s: the engine's sample count %lld is not a whole number of %d-sample control blocks", what,
                (long long)e->samples_processed, cb);
  for (int k = 0; k < e->n_presets(); ++k) {
    const af::ChainParams &o = e->presets[k].params;
    bool xf = false;
    for (int j = 0; j < o.n_eq_sections; ++j) xf = xf || o.eq[j].xf_remaining > 0;
    if (o.flags & af::kFlagDeesser)
      for (const af::DeEsserBandParams &b : o.deesser.bands)
        xf = xf || b.detector_hp.xf_remaining > 0 || b.detector_lp.xf_remaining > 0 || b.dynamic_eq.xf_remaining > 0;
    if (xf)
      return fail(AF_ERR_UNSUPPORTED, "%s: a coefficient crossfade is in flight in preset %d; its counters are shared by the preset's "
                                      "streams.  Process until it has ended", what, k);
  }
  if (!e->retune_ops.empty())
    return fail(AF_ERR_UNSUPPORTED, "%s: %d live-control state edits are pending; they apply to every stream of their preset at the "
                                    "next call", what, (int)e->retune_ops.size());
  return AF_OK;
}
int lifecycle_accepts(af_engine *e, const char *what, const int32_t *streams, int32_t n) {
  if (int rc = lifecycle_accepts_config(e, what, streams, n)) return rc;
  return lifecycle_accepts_state(e, what);
}

ss::PlaneView lifecycle_view(const af_engine *e) {
  ss::PlaneView v{};
  v.st64 = e->d_st64;
  v.st32 = e->d_st32;
  v.gate = e->d_gate;
  v.supp = e->supp.enabled ? e->supp.d_state.get() : nullptr;
  v.n_streams = e->n_streams;
  v.rows64 = e->n_f64;
  v.rows32_plane = e->n_f32;
  v.ring_cap = (e->n_f32 - af::kF32Fixed) / 2;
  return v;
}

void lifecycle_slots(af_engine *e, const int32_t *streams, int32_t n, std::vector<ss::Slot> &slots) {
  slots.resize((size_t)n);
  for (int32_t i = 0; i < n; ++i) {
    const int k = preset_of_stream(e, streams[i]);
    const int W = e->presets[k].proto.limiter.lookahead_samples + 1;
    slots[(size_t)i] = ss::Slot{streams[i], k, W, (int32_t)(e->samples_processed % W)};
  }
}

size_t round16(size_t b) { return (b + 15u) & ~(size_t)15u; }

// the staging pointers of a transfer of n streams inside e->life.d_stage, the slot list behind them
ss::TransferArgs lifecycle_transfer(af_engine *e, const ss::Shape &s, int32_t n) {
  ss::TransferArgs a{};
  a.v = lifecycle_view(e);
  unsigned char *base = e->life.d_stage;
  a.stage64 = reinterpret_cast<int64_t *>(base);
  a.stage32 = reinterpret_cast<float *>(base + ss::stage_f32_offset(s, n));
  a.stage_supp = s.suppressor ? reinterpret_cast<float *>(base + ss::stage_supp_offset(s, n)) : nullptr;
  a.slots = reinterpret_cast<const ss::Slot *>(base + round16(ss::stage_bytes(s, n)));
  a.n = n;
  a.words64 = ss::words64(s);
  a.rows32 = s.rows32;
  return a;
}
}  // namespace

int af_engine_restart_streams(af_engine *e, const int32_t *streams, int32_t n) {
  if (int rc = lifecycle_accepts(e, "af_engine_restart_streams", streams, n)) return rc;
  if (n == 0) return AF_OK;
  AF_HIP(e->use_device());
  hipStream_t stream = e->last_stream;
  // one upload: [prototype f64 columns | slot list | prototype f32 columns], then one launch; the host waits for neither
  const int n_presets = e->n_presets();
  const size_t b64 = sizeof(double) * (size_t)n_presets * e->n_f64, bsl = sizeof(ss::Slot) * (size_t)n;
  std::vector<unsigned char> host(round16(b64) + round16(bsl) + sizeof(float) * (size_t)n_presets * af::kF32Fixed, 0);
  double *p64 = reinterpret_cast<double *>(host.data());
  float *p32 = reinterpret_cast<float *>(host.data() + round16(b64) + round16(bsl));
  for (int k = 0; k < n_presets; ++k) initial_rows(e, k, p64 + (size_t)k * e->n_f64, p32 + (size_t)k * af::kF32Fixed);
  std::vector<ss::Slot> slots;
  lifecycle_slots(e, streams, n, slots);
  std::memcpy(host.data() + round16(b64), slots.data(), bsl);
  AF_HIP(e->life.d_stage.reserve_retiring(host.size(), e->retired, stream));
  AF_HIP(e->life.stager.upload(e->life.d_stage, host.data(), host.size(), stream));
  ss::RestartArgs a{};
  a.v = lifecycle_view(e);
  a.proto64 = reinterpret_cast<const double *>(e->life.d_stage.get());
  a.slots = reinterpret_cast<const ss::Slot *>(e->life.d_stage + round16(b64));
  a.proto32 = reinterpret_cast<const float *>(e->life.d_stage + round16(b64) + round16(bsl));
  a.n = n;
  a.n_presets = n_presets;
  AF_HIP(ss::launch_restart(a, stream));
  for (int32_t i = 0; i < n; ++i) e->life.set_origin(streams[i], e->samples_processed, e->n_streams);
  return AF_OK;
}

int af_engine_stream_state_size(af_engine *e, size_t *bytes) {
  if (!e || !bytes) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  *bytes = ss::blob_bytes(lifecycle_shape(e, 0));  // (the size depends on the engine's planes alone, not on the slot's preset)
  return AF_OK;
}

int af_engine_export_stream_state(af_engine *e, const int32_t *streams, int32_t n, void *blobs) {
  if (int rc = lifecycle_accepts_config(e, "af_engine_export_stream_state", streams, n)) return rc;
  if (n > 0 && !blobs) return fail(AF_ERR_INVALID_ARGUMENT, "af_engine_export_stream_state: blobs is null");
  if (int rc = lifecycle_accepts_state(e, "af_engine_export_stream_state")) return rc;
  if (n == 0) return AF_OK;
  AF_HIP(e->use_device());
  hipStream_t stream = e->last_stream;
  std::vector<ss::Shape> shapes((size_t)n);
  std::vector<int64_t> samples((size_t)n);
  for (int32_t i = 0; i < n; ++i) {
    shapes[(size_t)i] = lifecycle_shape(e, preset_of_stream(e, streams[i]));
    samples[(size_t)i] = e->samples_processed - e->life.origin_of(streams[i]);
  }
  const ss::Shape &s = shapes[0];
  const size_t stage = ss::stage_bytes(s, n), bsl = sizeof(ss::Slot) * (size_t)n;
  AF_HIP(e->life.d_stage.reserve_retiring(round16(stage) + bsl, e->retired, stream));
  std::vector<ss::Slot> slots;
  lifecycle_slots(e, streams, n, slots);
  AF_HIP(e->life.stager.upload(e->life.d_stage + round16(stage), slots.data(), bsl, stream));
  AF_HIP(ss::launch_export(lifecycle_transfer(e, s, n), stream));
  std::vector<unsigned char> host(stage);
  AF_HIP(hipMemcpyAsync(host.data(), e->life.d_stage, stage, hipMemcpyDeviceToHost, stream));
  AF_HIP(hipStreamSynchronize(stream));
  ss::stage_to_blobs(host.data(), n, shapes, samples, static_cast<unsigned char *>(blobs), ss::blob_bytes(s));
  return AF_OK;
}

int af_engine_import_stream_state(af_engine *e, const int32_t *streams, int32_t n, const void *blobs) {
  if (int rc = lifecycle_accepts_config(e, "af_engine_import_stream_state", streams, n)) return rc;
  if (n > 0 && !blobs) return fail(AF_ERR_INVALID_ARGUMENT, "af_engine_import_stream_state: blobs is null");
  if (n == 0) return lifecycle_accepts_state(e, "af_engine_import_stream_state");
  // every header against its destination slot, before anything is touched
  const ss::Shape s0 = lifecycle_shape(e, preset_of_stream(e, streams[0]));
  const size_t stride = ss::blob_bytes(s0);
  const unsigned char *src = static_cast<const unsigned char *>(blobs);
  std::vector<int64_t> samples((size_t)n);
  for (int32_t i = 0; i < n; ++i) {
    ss::BlobHeader h;
    std::memcpy(&h, src + (size_t)i * stride, sizeof h);
    const std::string msg = ss::check_header(h, lifecycle_shape(e, preset_of_stream(e, streams[i])));
    if (!msg.empty()) return fail(AF_ERR_INVALID_ARGUMENT, "af_engine_import_stream_state: blob %d for stream %d: %s", i, streams[i], msg.c_str());
    samples[(size_t)i] = h.samples;
  }
  if (int rc = lifecycle_accepts_state(e, "af_engine_import_stream_state")) return rc;
  AF_HIP(e->use_device());
  hipStream_t stream = e->last_stream;
  const size_t stage = ss::stage_bytes(s0, n), bsl = sizeof(ss::Slot) * (size_t)n;
  std::vector<unsigned char> host(round16(stage) + bsl, 0);
  ss::blobs_to_stage(src, stride, n, s0, host.data());
  std::vector<ss::Slot> slots;
  lifecycle_slots(e, streams, n, slots);
  std::memcpy(host.data() + round16(stage), slots.data(), bsl);
  AF_HIP(e->life.d_stage.reserve_retiring(host.size(), e->retired, stream));
  AF_HIP(e->life.stager.upload(e->life.d_stage, host.data(), host.size(), stream));
  AF_HIP(ss::launch_import(lifecycle_transfer(e, s0, n), stream));
  for (int32_t i = 0; i < n; ++i) e->life.set_origin(streams[i], e->samples_processed - samples[(size_t)i], e->n_streams);
  return AF_OK;
}

int af_engine_stream_samples_processed(const af_engine *e, int32_t stream, int64_t *samples) {
  if (!e || !samples) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (stream < 0 || stream >= e->n_streams) return fail(AF_ERR_INVALID_ARGUMENT, "stream %d out of range for %d streams", stream, e->n_streams);
  *samples = e->samples_processed - e->life.origin_of(stream);
  return AF_OK;
}

// ---- stateless helpers -----------------------------------------------------------------
int af_eq_magnitude_response(const double *freqs, size_t n, const double bands[10][3], double sample_rate,
                             double *out_db) {  // lib.rs:99-150
  if (!std::isfinite(sample_rate) || sample_rate <= 0.0)
    return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be finite and positive");
  if (!bands || (!freqs && n) || (!out_db && n)) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  const double nyquist = sample_rate / 2.0;
  for (int i = 0; i < af::kNumBands; ++i) {
    const double f = bands[i][0], g = bands[i][1], q = bands[i][2];
    if (!std::isfinite(f) || f <= 0.0 || f >= nyquist)
      return fail(AF_ERR_INVALID_ARGUMENT, "band %d frequency must be between 0 Hz and Nyquist", i);
    if (!std::isfinite(g)) return fail(AF_ERR_INVALID_ARGUMENT, "band %d gain must be finite", i);
    if (!std::isfinite(q) || q <= 0.0) return fail(AF_ERR_INVALID_ARGUMENT, "band %d Q must be finite and positive", i);
  }
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(freqs[i]) || freqs[i] < 0.0 || freqs[i] > nyquist)
      return fail(AF_ERR_INVALID_ARGUMENT, "response frequencies must be finite and between 0 Hz and Nyquist");
  af::EqProto eq(sample_rate);
  for (int i = 0; i < af::kNumBands; ++i) {
    eq.set_band_frequency(i, bands[i][0]);
    eq.set_band_gain(i, bands[i][1]);
    eq.set_band_q(i, bands[i][2]);
  }
  for (size_t i = 0; i < n; ++i) out_db[i] = eq.magnitude_db(freqs[i]);
  return AF_OK;
}

int af_eq_magnitude_response_v2(const double *freqs, size_t n, const af_eq_band_config bands[10], double sample_rate,
                                double *out_db) {  // lib.rs:152-212
  if (!std::isfinite(sample_rate) || sample_rate <= 0.0)
    return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be finite and positive");
  if (!bands || (!freqs && n) || (!out_db && n)) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  for (int i = 0; i < af::kNumBands; ++i)
    if (int rc = af_eq_band_config_validate(&bands[i], i, sample_rate)) return rc;
  const double nyquist = sample_rate / 2.0;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(freqs[i]) || freqs[i] < 0.0 || freqs[i] > nyquist)
      return fail(AF_ERR_INVALID_ARGUMENT, "response frequencies must be finite and between 0 Hz and Nyquist");
  af::EqProto eq(sample_rate);
  for (int i = 0; i < af::kNumBands; ++i) eq.set_band_config(i, to_cfg(bands[i]));
  for (size_t i = 0; i < n; ++i) out_db[i] = eq.magnitude_db(freqs[i]);
  return AF_OK;
}

int af_engine_eq_magnitude_response(const af_engine *e, const double *freqs, size_t n, double *out_db) {
  if (!e || (!freqs && n) || (!out_db && n)) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  for (size_t i = 0; i < n; ++i) out_db[i] = e->selected().proto.eq.magnitude_db(freqs[i]);
  return AF_OK;
}

}  // extern "C"

// af_api_internal.hpp: what af_noise_suppressor_reset needs from the engine
int af_engine_reinit_suppressor_state(af_engine *e) {
  if (!e) return fail(AF_ERR_INVALID_ARGUMENT, "engine is null");
  if (!e->started) return AF_OK;
  AF_HIP(e->use_device());
  AF_HIP(hipDeviceSynchronize());
  // the wet/dry smoothing state belongs to the wrapper, not to DenoiseState: it survives (rnnoise.rs:205-210)
  std::vector<float> smoothed((size_t)e->n_streams);
  float *const column = e->supp.d_state + af::SuppState::kSmoothedStrength;
  AF_HIP(hipMemcpy2D(smoothed.data(), sizeof(float), column, sizeof(float) * af::SuppState::kCount, sizeof(float), e->n_streams,
                     hipMemcpyDeviceToHost));
  AF_HIP(e->supp.reset_state(e->n_streams));
  AF_HIP(hipMemcpy2D(column, sizeof(float) * af::SuppState::kCount, smoothed.data(), sizeof(float), sizeof(float), e->n_streams,
                     hipMemcpyHostToDevice));
  return AF_OK;
}

