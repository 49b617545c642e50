// af_switches.hpp -- the library's run-time switches (environment variables for A/B and timing runs; none changes results) and
// the suppressor pipeline's window schedule.  Plain C++17, no HIP: host programs include it (tests/host/switches_main.cpp).
// The switches are read ONCE per process, by switches(); nothing else in csrc/ reads the environment, except
// resampler_variant_override, which a resampler calls when it is created.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace af {

constexpr int kSuppSpecBuffers = 3;  // spectrum / pitch-spectrum / record buffer sets of the suppressor (SuppressorHost::kSpecBuffers)

// The table: one field per switch, its default, its meaning.  (A new field also goes into same() of tests/host/switches_main.cpp.)
struct Switches {
  int roles = 0;                    // AF_ROLES: 0 AUTO never takes the role kernels; 1 compressor and limiter as role kernels; 2 only the limiter half
  int lim_cus = -1;                 // AF_LIM_CUS: CUs of the limiter half under AF_ROLES=2; -1 (unset) = as many as the chain
  bool chain_persistent = true;     // AF_CHAIN_PERSISTENT=0: one chain launch per window again; unset = on unless a tool serialises dispatches
  bool eq_offload = true;           // AF_EQ_OFFLOAD=0: the EQ stays inside the chain launches
  int eq_stream = -1;               // AF_EQ_STREAM: -1 (unset) lane-per-stream EQ with two waves per group; 1 one wave; 0 the systolic kernel everywhere
  bool eq_stream_power = true;      // AF_EQ_STREAM_POWER=0: auto-makeup windows keep the systolic kernel
  int staged = -1;                  // AF_STAGED: -1 (unset) AUTO decides; 0 AUTO stays off the stage pipeline; > 0 AUTO takes it where it serves
  int64_t stage_window = 2880;      // AF_STAGE_WINDOW: samples per window of the stage pipeline (rounded down to whole control blocks)
  int stage_skip = -1;              // AF_STAGE_SKIP=<StageId>: timing probe, that stage does nothing (results are garbage)
  bool deesser_dispatch = false;    // AF_DEESSER_DISPATCH=1: the de-esser's serial stages as a third dispatch per step
  int supp_window_frames = 0;       // AF_SUPP_WINDOW_FRAMES: frames per suppressor window; 0 (unset) = the engine's own
  bool supp_ramp = true;            // AF_SUPP_RAMP=0: uniform suppressor windows
  std::vector<int64_t> supp_ramp_list;  // AF_SUPP_RAMP_LIST=4,4,8,8,16: the opening windows, in frames
  int supp_ramp_end = -1;           // AF_SUPP_RAMP_END: -1 (unset) mirror the ramp at the call's end only in front of the stage pipeline; 0 never; else always
  int supp_depth = kSuppSpecBuffers;  // AF_SUPP_DEPTH: buffer sets the suppressor's pipeline uses, within [2, kSuppSpecBuffers]
  bool synth_split = true;          // AF_SYNTH_SPLIT=0: resynthesis + overlap-add stay behind the network on one stream
  int rnn_variant = 4;              // AF_RNN_VARIANT: waves (16 streams each) per network workgroup: 1, 2 or 4
  int auto_waves = 16;              // AF_AUTO_WAVES: waves of the auto-makeup token-ring kernel: 8, 12 or 16
  int cu_partition = -1;            // AF_CU_PARTITION: -1 (unset) automatic; 0 no CU masks; N the chain stream on N CUs
  bool serial_streams = false;      // AF_SERIAL_STREAMS (set, to anything): every stage on the caller's stream
  bool diag_skip_chain = false;     // AF_DIAG_SKIP_CHAIN (set, to anything): timing probe, the suppressor's windows without their chain
};

inline Switches parse_switches(const char *(*lookup)(const char *)) {
  Switches s;
  const auto num = [&](const char *name, int unset) {
    const char *v = lookup(name);
    return v ? std::atoi(v) : unset;
  };
  s.roles = num("AF_ROLES", 0);
  s.lim_cus = lookup("AF_LIM_CUS") ? std::max(0, num("AF_LIM_CUS", 0)) : -1;  // (a negative count was always no CUs)
  if (lookup("AF_CHAIN_PERSISTENT")) {
    s.chain_persistent = num("AF_CHAIN_PERSISTENT", 1) != 0;
  } else {
    // a launch that waits for kernels on other streams needs them to run beside it: off under counter collection of rocprofv3
    // `--pmc` and the runtime's blocking-launch debug switches
    for (const char *name : {"ROCPROF_COUNTER_COLLECTION", "AMD_SERIALIZE_KERNEL", "HIP_LAUNCH_BLOCKING", "CUDA_LAUNCH_BLOCKING"})
      if (num(name, 0) != 0) s.chain_persistent = false;
  }
  s.eq_offload = num("AF_EQ_OFFLOAD", 1) != 0;
  s.eq_stream = num("AF_EQ_STREAM", -1);
  s.eq_stream_power = num("AF_EQ_STREAM_POWER", 1) != 0;
  s.staged = num("AF_STAGED", -1);
  if (const char *v = lookup("AF_STAGE_WINDOW")) s.stage_window = std::atoll(v);
  s.stage_skip = num("AF_STAGE_SKIP", -1);
  s.deesser_dispatch = num("AF_DEESSER_DISPATCH", 0) != 0;
  if (lookup("AF_SUPP_WINDOW_FRAMES")) s.supp_window_frames = std::max(1, num("AF_SUPP_WINDOW_FRAMES", 1));
  s.supp_ramp = num("AF_SUPP_RAMP", 1) != 0;
  if (const char *v = lookup("AF_SUPP_RAMP_LIST"))
    for (const char *p = v; *p;) {  // (any single character separates two numbers)
      char *end = nullptr;
      const long n = std::strtol(p, &end, 10);
      if (end == p) break;
      if (n > 0) s.supp_ramp_list.push_back(n);
      p = *end ? end + 1 : end;
    }
  s.supp_ramp_end = num("AF_SUPP_RAMP_END", -1);
  s.supp_depth = std::min(kSuppSpecBuffers, std::max(2, num("AF_SUPP_DEPTH", kSuppSpecBuffers)));
  s.synth_split = num("AF_SYNTH_SPLIT", 1) != 0;
  s.rnn_variant = num("AF_RNN_VARIANT", 4);
  s.auto_waves = num("AF_AUTO_WAVES", 16);
  s.cu_partition = num("AF_CU_PARTITION", -1);
  s.serial_streams = lookup("AF_SERIAL_STREAMS") != nullptr;
  s.diag_skip_chain = lookup("AF_DIAG_SKIP_CHAIN") != nullptr;
  return s;
}

inline const Switches &switches() {
  static const Switches s = parse_switches([](const char *name) -> const char * { return std::getenv(name); });
  return s;
}

// AF_RESAMPLER_VARIANT=valu|mfma32|<anything else>: read when a resampler is created (tests set it inside the process)
inline void resampler_variant_override(int &variant) {
  if (const char *env = std::getenv("AF_RESAMPLER_VARIANT")) variant = std::strcmp(env, "valu") == 0 ? 1 : (std::strcmp(env, "mfma32") == 0 ? 2 : 0);
}

// ---- The suppressor pipeline's window schedule: a call of `frames` 480-sample frames as windows (first frame, frames).
struct SuppWindow { int64_t f0, nf; };

// a window must hold whole control blocks, or block boundaries (hence per-block semantics) would move: the least number of
// frames that is a whole number of `control_block`-sample blocks
inline int64_t supp_window_unit(int control_block) {
  int64_t unit = 1;
  while ((unit * 480) % control_block != 0) ++unit;
  return unit;
}

// `window_frames`: the engine's window length; `ramp_down`: whether the call closes with the mirror image of its opening
// (AF_SUPP_WINDOW_FRAMES and AF_SUPP_RAMP_END override the two).
inline std::vector<SuppWindow> supp_window_schedule(int64_t frames, int64_t unit, int window_frames, bool ramp_down, const Switches &sw) {
  if (sw.supp_window_frames > 0) window_frames = sw.supp_window_frames;  // tuning runs
  // Only the last control block of a call can be short, so the call is scheduled as aligned windows over its whole control
  // blocks plus one short final window for a ragged end: block boundaries do not move and the pipeline keeps its overlap.
  const int64_t aligned = (frames / unit) * unit, ragged = frames - aligned;
  int64_t window = std::max<int64_t>(unit, (window_frames / unit) * unit);
  window = std::min<int64_t>(window, std::max<int64_t>(aligned, unit));
  // The first chain launch cannot start before one window has been through the pre-pass, the analysis and the synthesis, and
  // the last chain launch runs after everything else is done: with uniform windows that is ~2.5 window times of a 20-window
  // call during which most of the chip idles.  So the call opens with short windows that double up to the full size and
  // closes with the mirror image (every size a whole number of control blocks).
  // The mirror image at the end of the call shortens what runs after the suppressor's last kernel -- when that is the stage
  // pipeline emptying.  Behind the token-ring kernel the chain is the longer side and trails the suppressor by more than a
  // window anyway: there the small windows only cost launches (189.3 against 190.0 ms per bench step).
  if (sw.supp_ramp_end >= 0) ramp_down = sw.supp_ramp_end != 0;
  std::vector<int64_t> up;
  if (!sw.supp_ramp_list.empty()) {
    for (int64_t n : sw.supp_ramp_list) up.push_back(std::min<int64_t>(window, ((n + unit - 1) / unit) * unit));
  } else {
    for (int64_t n = ((4 + unit - 1) / unit) * unit; n < window; n *= 2) up.push_back(n);
  }
  int64_t up_total = 0;
  for (int64_t n : up) up_total += n;
  std::vector<SuppWindow> wins;
  int64_t f = 0;
  const auto push = [&](int64_t n) { wins.push_back({f, n}); f += n; };
  if (sw.supp_ramp && !up.empty() && aligned >= 2 * up_total + 2 * window) {
    for (int64_t n : up) push(n);
    const int64_t body_end = ramp_down ? aligned - up_total : aligned;
    while (f < body_end) push(std::min<int64_t>(window, body_end - f));
    if (ramp_down)
      for (auto it = up.rbegin(); it != up.rend(); ++it) push(*it);
  } else {
    while (f < aligned) push(std::min<int64_t>(window, aligned - f));
  }
  if (ragged > 0) push(ragged);
  return wins;
}

}  // namespace af
