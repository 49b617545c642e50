// Stand-alone test of csrc/af_hip_resources.hpp against a fake HIP runtime defined in this file (it is not linked against
// the real one): allocations over malloc, one stream whose copies and event records run when the test drains it, and a
// switch that fails the k-th fallible call.  Built with -fsanitize=address,undefined by tests/test_host_resources.py.
#include "af_hip_resources.hpp"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <map>
#include <set>

namespace fake {
struct Ev { uint64_t recorded = 0, done = 0; };  // sequence number of the last record / the last record that has run
struct Op { Ev *ev; uint64_t seq; void *dst; const void *src; size_t bytes; };  // ev ? a record : a copy
std::deque<Op> queue;
std::map<void *, size_t> device, pinned;  // live allocations and their sizes
std::set<Ev *> events;
uint64_t seq = 0;
long calls = 0;           // every call into the fake
long fallible = 0;        // the calls that can be told to fail
long fail_at = 0;         // fail the fallible call with this number (1-based); 0 = none
long pinned_allocs = 0, blocking_waits = 0;
long script_fallible = 0;  // fallible calls of a whole run of script(), its destructors excluded
std::vector<Ev *> record_log, sync_log;
size_t last_pinned_bytes = 0;
bool query_fails_once = false;          // the next hipEventQuery reports an error other than "not ready"
hipError_t sticky = hipSuccess;         // what hipGetLastError returns and clears, as the runtime's

bool inject() { return ++fallible == fail_at; }
void run(const Op &op) {
  if (op.ev) op.ev->done = op.seq;
  else if (op.bytes) std::memcpy(op.dst, op.src, op.bytes);
}
void drain(size_t n_ops) {
  for (; n_ops && !queue.empty(); --n_ops) { run(queue.front()); queue.pop_front(); }
}
void drain_all() { drain(queue.size()); }
void reset() {
  queue.clear();
  record_log.clear();
  sync_log.clear();
  calls = fallible = fail_at = pinned_allocs = blocking_waits = 0;
  query_fails_once = false;
  sticky = hipSuccess;
}
bool nothing_live() { return device.empty() && pinned.empty() && events.empty(); }
}  // namespace fake

hipError_t hipMalloc(void **p, size_t n) {
  ++fake::calls;
  if (fake::inject()) return hipErrorOutOfMemory;
  *p = std::malloc(n ? n : 1);
  fake::device[*p] = n;
  return hipSuccess;
}
hipError_t hipFree(void *p) {
  ++fake::calls;
  if (!p) return hipSuccess;
  if (!fake::device.erase(p)) { std::fprintf(stderr, "hipFree of a pointer that is not live\n"); std::abort(); }
  std::free(p);
  return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t n, unsigned) {
  ++fake::calls;
  if (fake::inject()) return hipErrorOutOfMemory;
  *p = std::malloc(n ? n : 1);
  fake::pinned[*p] = n;
  ++fake::pinned_allocs;
  fake::last_pinned_bytes = n;
  return hipSuccess;
}
hipError_t hipHostFree(void *p) {  // (the real one waits for the device, too)
  ++fake::calls;
  fake::drain_all();
  if (!fake::pinned.erase(p)) { std::fprintf(stderr, "hipHostFree of a pointer that is not live\n"); std::abort(); }
  std::free(p);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *ev, unsigned) {
  ++fake::calls;
  if (fake::inject()) return hipErrorOutOfMemory;
  fake::Ev *e = new fake::Ev();
  fake::events.insert(e);
  *ev = reinterpret_cast<hipEvent_t>(e);
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *ev) { return hipEventCreateWithFlags(ev, 0); }
hipError_t hipEventDestroy(hipEvent_t ev) {
  ++fake::calls;
  fake::Ev *e = reinterpret_cast<fake::Ev *>(ev);
  if (!fake::events.erase(e)) { std::fprintf(stderr, "hipEventDestroy of an event that is not live\n"); std::abort(); }
  for (fake::Op &op : fake::queue)
    if (op.ev == e) op = fake::Op{nullptr, 0, nullptr, nullptr, 0};  // (a record of a destroyed event: nothing to run)
  delete e;
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t) {
  ++fake::calls;
  if (fake::inject()) return hipErrorUnknown;
  fake::Ev *e = reinterpret_cast<fake::Ev *>(ev);
  e->recorded = ++fake::seq;
  fake::queue.push_back(fake::Op{e, e->recorded, nullptr, nullptr, 0});
  fake::record_log.push_back(e);
  return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t ev) {
  ++fake::calls;
  if (std::exchange(fake::query_fails_once, false)) return fake::sticky = hipErrorUnknown;
  fake::Ev *e = reinterpret_cast<fake::Ev *>(ev);
  return e->done == e->recorded ? hipSuccess : hipErrorNotReady;
}
hipError_t hipEventSynchronize(hipEvent_t ev) {
  ++fake::calls;
  if (fake::inject()) return hipErrorUnknown;
  fake::Ev *e = reinterpret_cast<fake::Ev *>(ev);
  fake::sync_log.push_back(e);
  if (e->done != e->recorded) ++fake::blocking_waits;
  while (e->done != e->recorded) fake::drain(1);  // the stream runs up to the record
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) {
  ++fake::calls;
  *ms = 1.0f;
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) {
  ++fake::calls;
  if (fake::inject()) return hipErrorUnknown;
  fake::queue.push_back(fake::Op{nullptr, 0, dst, src, bytes});
  return hipSuccess;
}
hipError_t hipGetLastError(void) { ++fake::calls; return std::exchange(fake::sticky, hipSuccess); }
const char *hipGetErrorString(hipError_t) { return "fake"; }

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

static void test_reserve_retiring() {
  fake::reset();
  {
    af::RetireList retired;
    af::DeviceBuffer<char> b;
    const size_t need[4] = {100, 100, 101, 1000}, cap[4] = {100, 100, 150, 1000};
    void *old[2] = {nullptr, nullptr};
    for (int i = 0; i < 4; ++i) {
      void *before = b.get();
      CHECK(b.reserve_retiring(need[i], retired, nullptr) == hipSuccess);
      CHECK(b.bytes() == cap[i]);
      if (i >= 2) old[i - 2] = before;
    }
    CHECK(fake::blocking_waits == 0 && fake::sync_log.empty());  // growing never synchronises
    CHECK(retired.size() == 2 && fake::device.count(old[0]) && fake::device.count(old[1]));
    retired.collect(false);  // both events pending: nothing is freed
    CHECK(retired.size() == 2 && fake::device.count(old[0]) && fake::device.count(old[1]));
    fake::drain(1);  // the first record runs
    retired.collect(false);
    CHECK(retired.size() == 1 && !fake::device.count(old[0]) && fake::device.count(old[1]));
    retired.collect(true);
    CHECK(retired.size() == 0 && fake::device.size() == 1);
  }
  CHECK(fake::nothing_live());
}

// what collect() does with an error that is not "not ready", and the destructor with a wait that fails
static void test_retire_errors() {
  fake::reset();
  {
    af::RetireList retired;
    af::DeviceBuffer<char> b;
    CHECK(b.reserve_retiring(10, retired, nullptr) == hipSuccess && b.reserve_retiring(20, retired, nullptr) == hipSuccess);
    CHECK(b.reserve_retiring(40, retired, nullptr) == hipSuccess && retired.size() == 2);
    fake::drain_all();  // both records have run
    fake::query_fails_once = true;
    retired.collect(false);  // the first query fails: that buffer is kept, the runtime's sticky error is cleared
    CHECK(retired.size() == 1 && fake::device.size() == 2 && fake::sticky == hipSuccess);
    fake::fail_at = fake::fallible + 1;  // the destructor's wait for it fails: the buffer is freed all the same
  }
  CHECK(fake::nothing_live());
}

static void test_reserve_exact() {
  fake::reset();
  {
    af::DeviceBuffer<float> b;
    CHECK(b.reserve_exact(64) == hipSuccess && b.bytes() == 64 && b.get());
    CHECK(b.reserve_exact(32) == hipSuccess && b.bytes() == 64);
    fake::fail_at = fake::fallible + 1;
    CHECK(b.reserve_exact(128) == hipErrorOutOfMemory);
    CHECK(b.get() == nullptr && b.bytes() == 0 && fake::device.empty());
    CHECK(b.reserve_exact(16) == hipSuccess && b.bytes() == 16 && b.get());
    CHECK(b.keep_if(hipSuccess) == hipSuccess && b.get());  // first contents written: kept
    CHECK(b.keep_if(hipErrorUnknown) == hipErrorUnknown && b.get() == nullptr && b.bytes() == 0 && fake::device.empty());
  }
  CHECK(fake::nothing_live());
}

static void fill(unsigned char *p, size_t n, int tag) {
  for (size_t i = 0; i < n; ++i) p[i] = (unsigned char)(tag * 31 + i);
}
static bool holds(const unsigned char *p, size_t n, int tag) {
  for (size_t i = 0; i < n; ++i)
    if (p[i] != (unsigned char)(tag * 31 + i)) return false;
  return true;
}

static void test_pinned_slots() {
  fake::reset();
  {
    constexpr size_t kBytes = 64;
    af::DeviceBuffer<unsigned char> dst;
    CHECK(dst.reserve_exact(16 * 1024) == hipSuccess);
    af::PinnedSlots<4> slots;
    unsigned char src[1024];
    int n = 0;  // uploads so far; upload i goes to dst + i * kBytes
    auto upload = [&](size_t bytes) {
      fill(src, bytes, n);
      CHECK(slots.upload(dst.get() + n * kBytes, src, bytes, nullptr) == hipSuccess);
      std::memset(src, 0xee, sizeof src);  // the caller's source changes right away
      ++n;
    };
    for (int i = 0; i < 4; ++i) upload(kBytes);
    CHECK(fake::sync_log.empty() && fake::pinned_allocs == 1);
    upload(kBytes);  // the fifth: its slot is the first upload's
    CHECK(fake::sync_log.size() == 1 && fake::sync_log[0] == fake::record_log[0] && fake::blocking_waits == 1);
    fake::drain_all();
    for (int i = 0; i < 5; ++i) CHECK(holds(dst.get() + i * kBytes, kBytes, i));
    for (int i = 0; i < 4; ++i) upload(kBytes);  // every earlier copy has completed: no wait blocks
    CHECK(fake::blocking_waits == 1 && fake::pinned_allocs == 1);
    fake::drain_all();
    // growth: three copies in flight, then a request larger than a slot
    for (int i = 0; i < 3; ++i) upload(kBytes);
    const size_t syncs = fake::sync_log.size(), records = fake::record_log.size();
    const long waits = fake::blocking_waits;
    upload(kBytes + 1);
    CHECK(fake::blocking_waits == waits + 3);
    for (size_t k = 0; k < 3; ++k) {  // every slot in flight was waited for
      bool seen = false;
      for (size_t j = syncs; j < fake::sync_log.size(); ++j) seen |= fake::sync_log[j] == fake::record_log[records - 3 + k];
      CHECK(seen);
    }
    CHECK(fake::pinned_allocs == 2 && fake::pinned.size() == 1);
    CHECK(fake::last_pinned_bytes >= 4 * (kBytes + kBytes / 2));
    fake::drain_all();
    for (int i = 9; i < 12; ++i) CHECK(holds(dst.get() + i * kBytes, kBytes, i));
    CHECK(holds(dst.get() + 12 * kBytes, kBytes + 1, 12));
    upload(kBytes + kBytes / 2);  // fits the grown slot
    CHECK(fake::pinned_allocs == 2);
    // two ranges land back to back
    unsigned char a[12], b[5];
    fill(a, sizeof a, 100);
    fill(b, sizeof b, 101);
    unsigned char *at = dst.get() + 8 * 1024;
    CHECK(slots.upload(at, a, sizeof a, b, sizeof b, nullptr) == hipSuccess);
    std::memset(a, 0, sizeof a);
    std::memset(b, 0, sizeof b);
    fake::drain_all();
    CHECK(holds(at, 12, 100) && holds(at + 12, 5, 101));
  }
  CHECK(fake::nothing_live());
}

static void test_timed_span() {
  fake::reset();
  {
    af::TimedSpan span;
    double ms = -1.0;
    CHECK(span.elapsed_ms(&ms) == hipSuccess && ms == 0.0 && fake::calls == 0);
    fake::fail_at = fake::fallible + 2;  // the second event's creation
    CHECK(span.begin(nullptr) != hipSuccess && !span.used());
    const long calls = fake::calls;
    ms = -1.0;
    CHECK(span.elapsed_ms(&ms) == hipSuccess && ms == 0.0 && fake::calls == calls);
    CHECK(span.begin(nullptr) == hipSuccess && span.end(nullptr) == hipSuccess && span.used());
    CHECK(fake::events.size() == 2);
    CHECK(span.elapsed_ms(&ms) == hipSuccess && ms == 1.0);
    af::EventChain chain;
    for (int i = 0; i < 3; ++i) CHECK(chain.mark(nullptr) == hipSuccess);
    chain.restart();
    for (int i = 0; i < 3; ++i) CHECK(chain.mark(nullptr) == hipSuccess);
    CHECK(chain.marks() == 3 && fake::events.size() == 5);
    CHECK(chain.wait_last() == hipSuccess && chain.elapsed(0, 2, &ms) == hipSuccess && ms == 1.0);
  }
  CHECK(fake::nothing_live());
}

// construct each owner, grow twice, upload six times, retire, collect, destroy; stops at the first error
static hipError_t script() {
#define TRY(expr)                                        \
  do {                                                   \
    if (hipError_t err__ = (expr); err__ != hipSuccess) return err__; \
  } while (0)
  af::DeviceBuffer<unsigned char> dst;
  af::RetireList retired;
  af::DeviceBuffer<> scratch;
  af::DeviceBuffer<double> staging;
  af::PinnedSlots<4> slots;
  af::TimedSpan span;
  af::EventChain chain;
  unsigned char src[96] = {};
  TRY(dst.reserve_exact(1024));
  TRY(staging.reserve_exact(64));
  TRY(staging.reserve_exact(256));
  TRY(span.begin(nullptr));
  TRY(chain.mark(nullptr));
  TRY(scratch.reserve_retiring(100, retired, nullptr));
  TRY(scratch.reserve_retiring(200, retired, nullptr));
  TRY(scratch.reserve_retiring(400, retired, nullptr));
  for (int i = 0; i < 6; ++i) TRY(slots.upload(dst.get() + 96 * i, src, i < 5 ? 64 : 96, nullptr));
  TRY(chain.mark(nullptr));
  TRY(span.end(nullptr));
  void *loose = nullptr;
  TRY(hipMalloc(&loose, 32));
  if (hipError_t err = retired.retire(loose, nullptr); err != hipSuccess) {
    (void)hipFree(loose);  // retire() takes the pointer over only when it succeeds
    return err;
  }
  retired.collect(false);
  double ms = 0.0;
  TRY(span.elapsed_ms(&ms));
  TRY(chain.wait_last());
  fake::script_fallible = fake::fallible;
  return hipSuccess;
#undef TRY
}

static void test_failure_sweep() {
  fake::reset();
  CHECK(script() == hipSuccess && fake::nothing_live());
  const long K = fake::script_fallible;
  CHECK(K > 30);
  for (long k = 1; k <= K; ++k) {
    fake::reset();
    fake::fail_at = k;
    CHECK(script() != hipSuccess);
    CHECK(fake::fallible >= k);
    CHECK(fake::nothing_live());
  }
}

int main() {
  test_reserve_retiring();
  test_retire_errors();
  test_reserve_exact();
  test_pinned_slots();
  test_timed_span();
  test_failure_sweep();
  const double samples[6] = {0.0, 1.0, HUGE_VAL, 2.0, 3.0, 4.0};  // 2 rows of 2, 3 apart: the infinity is in no row
  CHECK(af::check_finite(samples, 2, 2, 3) && !af::check_finite(samples, 2, 3, 3));
  std::puts("resources: ok");
  return 0;
}
