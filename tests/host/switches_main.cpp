// Stand-alone test of csrc/af_switches.hpp: parse_switches through a fake environment (every default, every switch whose
// parsing has a trap, the removed names), and the suppressor pipeline's window schedule over a sweep of call lengths, control
// blocks and window lengths plus literal schedules.  No HIP, no GPU.  Built with -fsanitize=address,undefined by
// tests/test_host_switches.py.
#include "af_switches.hpp"

#include <cstdio>
#include <map>
#include <string>

namespace {
std::map<std::string, std::string> env;
const char *lookup(const char *name) {
  const auto it = env.find(name);
  return it == env.end() ? nullptr : it->second.c_str();
}
af::Switches parse(std::map<std::string, std::string> e) {
  env = std::move(e);
  return af::parse_switches(lookup);
}
int failures = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);          \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

// every field of Switches by hand: a field added to the struct changes its size and has to be added here
static_assert(sizeof(af::Switches) == 80 + sizeof(std::vector<int64_t>), "af::Switches changed: update same() below, then this size");
bool same(const af::Switches &a, const af::Switches &b) {
  return a.roles == b.roles && a.lim_cus == b.lim_cus && a.chain_persistent == b.chain_persistent && a.eq_offload == b.eq_offload &&
         a.eq_stream == b.eq_stream && a.eq_stream_power == b.eq_stream_power && a.staged == b.staged && a.stage_window == b.stage_window &&
         a.stage_skip == b.stage_skip && a.deesser_dispatch == b.deesser_dispatch && a.supp_window_frames == b.supp_window_frames &&
         a.supp_ramp == b.supp_ramp && a.supp_ramp_list == b.supp_ramp_list && a.supp_ramp_end == b.supp_ramp_end &&
         a.supp_depth == b.supp_depth && a.synth_split == b.synth_split && a.rnn_variant == b.rnn_variant && a.auto_waves == b.auto_waves &&
         a.cu_partition == b.cu_partition && a.serial_streams == b.serial_streams && a.diag_skip_chain == b.diag_skip_chain;
}

void test_defaults() {
  const af::Switches s = parse({});
  CHECK(same(s, af::Switches{}));
  CHECK(s.roles == 0 && s.lim_cus == -1 && s.chain_persistent && s.eq_offload && s.eq_stream == -1 && s.eq_stream_power);
  CHECK(s.staged == -1 && s.stage_window == 2880 && s.stage_skip == -1 && !s.deesser_dispatch);
  CHECK(s.supp_window_frames == 0 && s.supp_ramp && s.supp_ramp_list.empty() && s.supp_ramp_end == -1 && s.supp_depth == af::kSuppSpecBuffers);
  CHECK(s.synth_split && s.rnn_variant == 4 && s.auto_waves == 16 && s.cu_partition == -1 && !s.serial_streams && !s.diag_skip_chain);
}

void test_traps() {
  // presence tests: set to 0 they still count
  CHECK(parse({{"AF_SERIAL_STREAMS", "0"}}).serial_streams);
  CHECK(parse({{"AF_SERIAL_STREAMS", ""}}).serial_streams);
  CHECK(parse({{"AF_DIAG_SKIP_CHAIN", "0"}}).diag_skip_chain);
  CHECK(parse({{"AF_DIAG_SKIP_CHAIN", "1"}}).diag_skip_chain);
  // AF_EQ_STREAM: unset two waves, 1 one wave, 0 systolic everywhere
  CHECK(parse({{"AF_EQ_STREAM", "1"}}).eq_stream == 1);
  CHECK(parse({{"AF_EQ_STREAM", "0"}}).eq_stream == 0);
  CHECK(parse({{"AF_EQ_STREAM", "2"}}).eq_stream != 0 && parse({{"AF_EQ_STREAM", "2"}}).eq_stream != 1);
  CHECK(parse({}).eq_stream != 0 && parse({}).eq_stream != 1);
  // AF_STAGED: unset, 0, > 0
  CHECK(parse({{"AF_STAGED", "0"}}).staged == 0);
  CHECK(parse({{"AF_STAGED", "1"}}).staged > 0);
  CHECK(parse({}).staged < 0);
  // AF_SUPP_RAMP_END: unset, 0, else
  CHECK(parse({{"AF_SUPP_RAMP_END", "0"}}).supp_ramp_end == 0);
  CHECK(parse({{"AF_SUPP_RAMP_END", "1"}}).supp_ramp_end > 0);
  CHECK(parse({}).supp_ramp_end < 0);
  // AF_CHAIN_PERSISTENT: unset means on, unless a tool that serialises dispatches is announced; set, it decides
  CHECK(!parse({{"AF_CHAIN_PERSISTENT", "0"}}).chain_persistent);
  CHECK(parse({{"AF_CHAIN_PERSISTENT", "1"}}).chain_persistent);
  for (const char *tool : {"ROCPROF_COUNTER_COLLECTION", "AMD_SERIALIZE_KERNEL", "HIP_LAUNCH_BLOCKING", "CUDA_LAUNCH_BLOCKING"}) {
    CHECK(!parse({{tool, "1"}}).chain_persistent);
    CHECK(!parse({{tool, "3"}}).chain_persistent);
    CHECK(parse({{tool, "0"}}).chain_persistent);
    CHECK(parse({{tool, ""}}).chain_persistent);
    CHECK(parse({{tool, "1"}, {"AF_CHAIN_PERSISTENT", "1"}}).chain_persistent);
    CHECK(!parse({{tool, "0"}, {"AF_CHAIN_PERSISTENT", "0"}}).chain_persistent);
  }
  // AF_SUPP_RAMP_LIST: any single character between numbers; entries <= 0 are dropped; it ends at what is no number
  CHECK((parse({{"AF_SUPP_RAMP_LIST", "4,4,8,8,16"}}).supp_ramp_list == std::vector<int64_t>{4, 4, 8, 8, 16}));
  CHECK((parse({{"AF_SUPP_RAMP_LIST", "4:8 16;32"}}).supp_ramp_list == std::vector<int64_t>{4, 8, 16, 32}));
  CHECK((parse({{"AF_SUPP_RAMP_LIST", "4,0,-2,8"}}).supp_ramp_list == std::vector<int64_t>{4, 8}));
  CHECK((parse({{"AF_SUPP_RAMP_LIST", "4,,8"}}).supp_ramp_list == std::vector<int64_t>{4}));
  CHECK((parse({{"AF_SUPP_RAMP_LIST", "4,8,"}}).supp_ramp_list == std::vector<int64_t>{4, 8}));
  CHECK(parse({{"AF_SUPP_RAMP_LIST", ""}}).supp_ramp_list.empty());
  // AF_SUPP_DEPTH within [2, kSuppSpecBuffers]
  CHECK(parse({{"AF_SUPP_DEPTH", "0"}}).supp_depth == 2);
  CHECK(parse({{"AF_SUPP_DEPTH", "1"}}).supp_depth == 2);
  CHECK(parse({{"AF_SUPP_DEPTH", "2"}}).supp_depth == 2);
  CHECK(parse({{"AF_SUPP_DEPTH", "3"}}).supp_depth == 3);
  CHECK(parse({{"AF_SUPP_DEPTH", "9"}}).supp_depth == af::kSuppSpecBuffers);
  // AF_CU_PARTITION: 0 no masks, N forces N, unset automatic
  CHECK(parse({{"AF_CU_PARTITION", "0"}}).cu_partition == 0);
  CHECK(parse({{"AF_CU_PARTITION", "24"}}).cu_partition == 24);
  CHECK(parse({}).cu_partition < 0);
  // the plain ones
  CHECK(parse({{"AF_ROLES", "2"}}).roles == 2);
  CHECK(parse({{"AF_LIM_CUS", "16"}}).lim_cus == 16);
  CHECK(parse({{"AF_LIM_CUS", "0"}}).lim_cus == 0);
  CHECK(parse({{"AF_LIM_CUS", "-4"}}).lim_cus == 0);
  CHECK(!parse({{"AF_EQ_OFFLOAD", "0"}}).eq_offload && parse({{"AF_EQ_OFFLOAD", "1"}}).eq_offload);
  CHECK(!parse({{"AF_EQ_STREAM_POWER", "0"}}).eq_stream_power);
  CHECK(parse({{"AF_STAGE_WINDOW", "960"}}).stage_window == 960 && parse({{"AF_STAGE_WINDOW", "0"}}).stage_window == 0);
  CHECK(parse({{"AF_STAGE_SKIP", "5"}}).stage_skip == 5);
  CHECK(parse({{"AF_DEESSER_DISPATCH", "1"}}).deesser_dispatch && !parse({{"AF_DEESSER_DISPATCH", "0"}}).deesser_dispatch);
  CHECK(parse({{"AF_SUPP_WINDOW_FRAMES", "24"}}).supp_window_frames == 24 && parse({{"AF_SUPP_WINDOW_FRAMES", "0"}}).supp_window_frames == 1);
  CHECK(!parse({{"AF_SUPP_RAMP", "0"}}).supp_ramp && parse({{"AF_SUPP_RAMP", "1"}}).supp_ramp);
  CHECK(!parse({{"AF_SYNTH_SPLIT", "0"}}).synth_split);
  CHECK(parse({{"AF_RNN_VARIANT", "1"}}).rnn_variant == 1);
  CHECK(parse({{"AF_AUTO_WAVES", "12"}}).auto_waves == 12);
}

void test_removed_names() {
  const af::Switches s = parse({{"AF_EQ_PARTS", "2"}, {"AF_EQ_STREAM_OFF", "1"}, {"AF_EQ_ON_FIN", "1"}, {"AF_RNN_STREAM", "1"},
                                {"AF_ORDER_PITCH", "1"}, {"AF_CU_PATTERN", "2"}, {"AF_STATS_CLEAR", "window"},
                                {"AF_DIAG_NO_CHAIN_KERNEL", "1"}, {"AF_SYNTH_FUSED", "0"}, {"AF_PITCHSEARCH4", "0"}});
  CHECK(same(s, af::Switches{}));
}

std::vector<int64_t> sizes(const std::vector<af::SuppWindow> &wins) {
  std::vector<int64_t> v;
  for (const af::SuppWindow &w : wins) v.push_back(w.nf);
  return v;
}

void test_schedule_properties() {
  const std::vector<std::map<std::string, std::string>> envs = {{}, {{"AF_SUPP_RAMP", "0"}}, {{"AF_SUPP_RAMP_LIST", "4,4,8,8,16"}}};
  long points = 0;
  for (const auto &e : envs) {
    const af::Switches sw = parse(e);
    for (int cb : {64, 128, 256, 480, 512, 960}) {
      int64_t unit = 1;  // the least u for which u * 480 is divisible by cb
      while ((unit * 480) % cb != 0) ++unit;
      CHECK(af::supp_window_unit(cb) == unit);
      for (int window_frames : {1, 4, 20, 64})
        for (int ramp_down = 0; ramp_down < 2; ++ramp_down)
          for (int64_t frames = 0; frames <= 400; ++frames) {
            const std::vector<af::SuppWindow> wins = af::supp_window_schedule(frames, unit, window_frames, ramp_down != 0, sw);
            const int64_t full = std::max<int64_t>(unit, (window_frames / unit) * unit);
            int64_t at = 0;
            bool ok = true;
            for (size_t i = 0; i < wins.size(); ++i) {
              ok = ok && wins[i].f0 == at && wins[i].nf > 0;                               // in order, no gap, no empty window
              ok = ok && (wins[i].nf % unit == 0 || (i + 1 == wins.size() && wins[i].nf < unit));  // whole control blocks but for a ragged end
              ok = ok && wins[i].nf <= full;
              at += wins[i].nf;
            }
            ok = ok && at == frames;
            if (!ok) {
              std::printf("schedule property failed: frames %lld cb %d window_frames %d ramp_down %d env %zu\n", (long long)frames, cb,
                          window_frames, ramp_down, e.size());
              ++failures;
            }
            ++points;
          }
    }
  }
  std::printf("schedule sweep: %ld points\n", points);
}

// literal schedules (window sizes in frames), as the engine scheduled these calls before the schedule became a function
void test_schedule_literals() {
  using V = std::vector<int64_t>;
  const af::Switches d = parse({});
  CHECK((sizes(af::supp_window_schedule(100, 1, 20, false, d)) == V{4, 8, 16, 20, 20, 20, 12}));
  CHECK((sizes(af::supp_window_schedule(100, 1, 20, true, d)) == V{4, 8, 16, 20, 20, 4, 16, 8, 4}));
  V long_call{4, 8};  // 1000 frames in control blocks of 128 samples (unit 4): 4, 8, sixty-one full windows, the rest
  long_call.insert(long_call.end(), 61, 16);
  long_call.push_back(12);
  CHECK(sizes(af::supp_window_schedule(1000, af::supp_window_unit(128), 16, false, d)) == long_call);
  CHECK((sizes(af::supp_window_schedule(50, 1, 20, true, d)) == V{20, 20, 10}));                                     // too short for a ramp
  CHECK((sizes(af::supp_window_schedule(101, af::supp_window_unit(256), 20, false, d)) == V{8, 16, 16, 16, 16, 16, 8, 5}));  // unit 8, ragged end
  CHECK((sizes(af::supp_window_schedule(7, af::supp_window_unit(512), 64, true, d)) == V{7}));                          // shorter than one unit (16)
  CHECK((sizes(af::supp_window_schedule(100, 1, 20, true, parse({{"AF_SUPP_RAMP", "0"}}))) == V{20, 20, 20, 20, 20}));
  CHECK((sizes(af::supp_window_schedule(200, 1, 20, false, parse({{"AF_SUPP_RAMP_LIST", "4,4,8,8,16"}}))) ==
         V{4, 4, 8, 8, 16, 20, 20, 20, 20, 20, 20, 20, 20}));
  CHECK((sizes(af::supp_window_schedule(100, 1, 20, true, parse({{"AF_SUPP_RAMP_END", "0"}}))) == V{4, 8, 16, 20, 20, 20, 12}));
  CHECK((sizes(af::supp_window_schedule(100, 1, 20, false, parse({{"AF_SUPP_RAMP_END", "1"}}))) == V{4, 8, 16, 20, 20, 4, 16, 8, 4}));
  CHECK((sizes(af::supp_window_schedule(100, 1, 20, false, parse({{"AF_SUPP_WINDOW_FRAMES", "40"}}))) == V{40, 40, 20}));
  CHECK(af::supp_window_schedule(0, 1, 16, true, d).empty());
}
}  // namespace

int main() {
  test_defaults();
  test_traps();
  test_removed_names();
  test_schedule_properties();
  test_schedule_literals();
  if (failures) {
    std::printf("switches: %d failures\n", failures);
    return 1;
  }
  std::printf("switches: ok\n");
  return 0;
}
