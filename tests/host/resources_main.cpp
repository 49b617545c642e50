// Stand-alone test of csrc/af_hip_resources.hpp against the fake HIP runtime of fake_hip_runtime.hpp (it is not linked against
// the real one).  Built with -fsanitize=address,undefined by tests/test_host_resources.py.
#include "af_hip_resources.hpp"
#include "fake_hip_runtime.hpp"

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

struct Block { int32_t a[5]; double b; };  // (padding included: sync() compares bytes, the tests fill every one)
static Block block(int tag) {
  Block v;
  std::memset(&v, tag, sizeof v);
  return v;
}
static bool same(const Block *dev, const Block *src, size_t count) { return std::memcmp(dev, src, count * sizeof(Block)) == 0; }

static void test_mirrored_sync() {
  fake::reset();
  {
    af::Mirrored<Block> m;
    af::PinnedSlots<4> slots;
    bool up = true;
    Block src[3] = {block(1), block(2), block(3)};
    CHECK(m.sync(src, 3, slots, nullptr, &up) == hipErrorInvalidValue && !up);  // no room yet: refused, nothing written
    CHECK(m.reserve(3) == hipSuccess && m.get() && fake::device.size() == 1);
    CHECK(m.sync(src, 3, slots, nullptr, &up) == hipSuccess && up);              // first use
    fake::drain_all();
    CHECK(same(m.get(), src, 3));
    const long calls = fake::calls;
    CHECK(m.sync(src, 3, slots, nullptr, &up) == hipSuccess && !up && fake::calls == calls);  // identical: no runtime call at all
    src[1] = block(7);
    CHECK(m.sync(src, 3, slots, nullptr, &up) == hipSuccess && up);              // one block differs
    CHECK(m.sync(src, 2, slots, nullptr, &up) == hipSuccess && up);              // a different count is different contents
    CHECK(m.sync(src, 2, slots, nullptr, &up) == hipSuccess && !up);
    m.invalidate();
    CHECK(m.sync(src, 2, slots, nullptr, &up) == hipSuccess && up);
    CHECK(m.reserve(2) == hipSuccess && m.sync(src, 2, slots, nullptr, &up) == hipSuccess && !up);  // fits: the mirror holds
    Block *before = m.get();
    fake::drain_all();
    CHECK(m.reserve(8) == hipSuccess && m.get() && fake::device.size() == 1 && !fake::device.count(before));
    CHECK(m.sync(src, 2, slots, nullptr, &up) == hipSuccess && up);              // reallocated: the new buffer holds nothing yet
    // a slot of the array rewritten in turn: the mirror of the front cannot vouch for the array any more
    const Block window[2] = {block(9), block(10)};
    CHECK(m.send(7, window, 2, slots, nullptr) == hipErrorInvalidValue);         // past the end: refused
    CHECK(m.send(6, window, 2, slots, nullptr) == hipSuccess);
    CHECK(m.sync(src, 2, slots, nullptr, &up) == hipSuccess && up);
    fake::drain_all();
    CHECK(same(m.get(), src, 2) && same(m.get() + 6, window, 2));
    Block *const as_pointer = m;
    CHECK(as_pointer == m.get());
  }
  CHECK(fake::nothing_live());
}

// Every fallible call inside a sync() fails in turn: the mirror must not claim what the device never received.
static void test_mirrored_failures() {
  const Block old_src[2] = {block(1), block(2)}, src[2] = {block(3), block(4)};
  // `grow`: the upload also has to make the pinned allocation (a request larger than the slots so far)
  for (int grow = 0; grow < 2; ++grow) {
    long fallible_calls = 0;
    for (long k = 0; k == 0 || k <= fallible_calls; ++k) {  // k = 0: the run that counts them
      fake::reset();
      {
        af::Mirrored<Block> m;
        af::PinnedSlots<2> slots;
        bool up = false;
        CHECK(m.reserve(2) == hipSuccess);
        if (!grow) CHECK(m.sync(old_src, 2, slots, nullptr, &up) == hipSuccess && up);
        const long before = fake::fallible;
        if (k) fake::fail_at = before + k;
        const hipError_t err = m.sync(src, 2, slots, nullptr, &up);
        if (k == 0) {
          CHECK(err == hipSuccess && up);
          fallible_calls = fake::fallible - before;
          CHECK(fallible_calls >= (grow ? 4 : 2));  // [pinned allocation, event creation,] copy, record
        } else {
          CHECK(err != hipSuccess && !up);
          fake::fail_at = 0;
          CHECK(m.sync(src, 2, slots, nullptr, &up) == hipSuccess && up);  // the same contents again: uploaded again
        }
        CHECK(m.sync(src, 2, slots, nullptr, &up) == hipSuccess && !up);
        fake::drain_all();
        CHECK(same(m.get(), src, 2));
      }
      CHECK(fake::nothing_live());
    }
  }
}

static void test_stream() {
  fake::reset();
  {
    af::Stream none;  // empty: no call at all
    CHECK(!none.get());
  }
  CHECK(fake::calls == 0);
  hipStream_t callers = nullptr;
  CHECK(fake::create_stream(&callers) == hipSuccess);  // a stream of the caller's
  {
    af::Stream owned;
    CHECK(owned.create() == hipSuccess && owned.get() && fake::streams.size() == 2);
    const hipStream_t handle = owned;
    CHECK(handle == owned.get());
    af::Stream moved(std::move(owned));  // the moved-from owner is empty and destroys nothing
    CHECK(!owned.get() && moved.get() == handle);
    owned.reset();
    CHECK(fake::stream_destroys == 0);
    af::Stream masked;
    const uint32_t mask[2] = {0xffu, 0u};
    fake::fail_at = fake::fallible + 1;
    CHECK(masked.create_with_cu_mask(2, mask) != hipSuccess && !masked.get());  // a failed creation leaves it empty
    CHECK(masked.create_with_cu_mask(2, mask) == hipSuccess && masked.get() && fake::streams.size() == 3);
    masked = std::move(moved);  // what it held is destroyed, once
    CHECK(fake::stream_destroys == 1 && fake::streams.size() == 2 && masked.get() == handle);
    af::Stream alias;
    alias.borrow(callers);
    CHECK(alias.get() == callers);
    af::Stream alias2(std::move(alias));
    alias2.reset();  // a borrowed stream is never destroyed
    CHECK(fake::stream_destroys == 1 && fake::streams.count(callers));
    alias2.borrow(callers);
    masked.borrow(callers);  // borrowing lets go of the owned stream
    CHECK(fake::stream_destroys == 2 && !fake::streams.count(handle));
    CHECK(masked.create() == hipSuccess && masked.get() != callers);  // ... and creating lets go of the alias, destroying nothing
    CHECK(fake::stream_destroys == 2);
  }
  CHECK(fake::stream_destroys == 3 && fake::streams.size() == 1 && fake::streams.count(callers));
  CHECK(hipStreamDestroy(callers) == hipSuccess && fake::nothing_live());
}

// construct each owner, grow twice, upload six times, retire, collect, destroy; stops at the first error
static hipError_t script() {
#define TRY(expr)                                        \
  do {                                                   \
    if (hipError_t err__ = (expr); err__ != hipSuccess) return err__; \
  } while (0)
  af::DeviceBuffer<unsigned char> dst;
  af::Mirrored<Block> mirror;  // (ahead of the slots: their destructor lets the queued copies run)
  af::RetireList retired;
  af::DeviceBuffer<> scratch;
  af::DeviceBuffer<double> staging;
  af::PinnedSlots<4> slots;
  af::TimedSpan span;
  af::EventChain chain;
  af::Stream plain, masked;
  const Block blocks[2] = {block(1), block(2)};
  const uint32_t mask = 1u;
  unsigned char src[96] = {};
  TRY(plain.create());
  TRY(masked.create_with_cu_mask(1, &mask));
  TRY(mirror.reserve(2));
  TRY(mirror.sync(blocks, 2, slots, plain));
  TRY(mirror.send(1, blocks, 1, slots, masked));
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
  test_mirrored_sync();
  test_mirrored_failures();
  test_stream();
  test_failure_sweep();
  const double samples[6] = {0.0, 1.0, HUGE_VAL, 2.0, 3.0, 4.0};  // 2 rows of 2, 3 apart: the infinity is in no row
  CHECK(af::check_finite(samples, 2, 2, 3) && !af::check_finite(samples, 2, 3, 3));
  std::puts("resources: ok");
  return 0;
}
