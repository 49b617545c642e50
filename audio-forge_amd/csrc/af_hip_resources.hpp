// af_hip_resources.hpp -- move-only owners of what the host side of the C ABI takes from the HIP runtime: device buffers,
// pinned staging slots, events, streams.  Host only, header only.  Every hipMalloc / hipFree / hipHostMalloc / hipHostFree /
// hipEventCreate / hipEventDestroy / hipStreamCreate / hipStreamDestroy of the ABI sources is in this file.  None of the
// owners knows a device: the object that holds them makes its device current (and synchronises it) before they are used or
// destroyed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

namespace af {

class Event {
 public:
  Event() = default;
  Event(Event &&o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
  Event &operator=(Event &&o) noexcept {
    if (this != &o) { reset(); ev_ = std::exchange(o.ev_, nullptr); }
    return *this;
  }
  ~Event() { reset(); }
  // no-op when the event exists; after a failure there is none and a later call tries again
  hipError_t create(unsigned flags = hipEventDefault) {
    if (ev_) return hipSuccess;
    const hipError_t err = hipEventCreateWithFlags(&ev_, flags);
    if (err != hipSuccess) ev_ = nullptr;
    return err;
  }
  void reset() {
    if (ev_) (void)hipEventDestroy(ev_);
    ev_ = nullptr;
  }
  hipEvent_t get() const { return ev_; }
  explicit operator bool() const { return ev_ != nullptr; }

 private:
  hipEvent_t ev_ = nullptr;
};

// Device buffers that had to grow while queued work may still read them: each is kept until an event recorded on the stream
// of the call that replaced it has completed, and freed by a later collect() or the destructor.
class RetireList {
 public:
  RetireList() = default;
  RetireList(RetireList &&) = default;
  RetireList &operator=(RetireList &&) = default;
  ~RetireList() {
    collect(true);
    for (Item &it : items_) (void)hipFree(it.p);  // (a wait that failed: the owner has synchronised the device)
  }
  // takes `p` over only when it succeeds
  hipError_t retire(void *p, hipStream_t stream) {
    Event ev;
    if (hipError_t err = ev.create(hipEventDisableTiming); err != hipSuccess) return err;
    if (hipError_t err = hipEventRecord(ev.get(), stream); err != hipSuccess) return err;
    items_.push_back(Item{p, std::move(ev)});
    return hipSuccess;
  }
  // free the buffers whose last reader has ended (`wait_for_all`: wait for them)
  void collect(bool wait_for_all) {
    size_t kept = 0;
    for (Item &it : items_) {
      const hipError_t q = wait_for_all ? hipEventSynchronize(it.ev.get()) : hipEventQuery(it.ev.get());
      if (q == hipSuccess) {
        (void)hipFree(it.p);
      } else {
        if (q != hipErrorNotReady) (void)hipGetLastError();
        if (&items_[kept] != &it) items_[kept] = std::move(it);
        ++kept;
      }
    }
    items_.resize(kept);
  }
  size_t size() const { return items_.size(); }

 private:
  struct Item { void *p = nullptr; Event ev; };
  std::vector<Item> items_;
};

// A device allocation and its capacity in bytes; converts to the T* it holds.
template <class T = void>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
    if (this != &o) { release(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
    return *this;
  }
  ~DeviceBuffer() { release(); }
  T *get() const { return static_cast<T *>(p_); }
  operator T *() const { return get(); }
  size_t bytes() const { return bytes_; }
  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  // Around the call that writes a fresh buffer's first contents: when it failed the buffer is released, so that "allocated"
  // goes on meaning "initialised" and the next call allocates and writes again.
  hipError_t keep_if(hipError_t written) {
    if (written != hipSuccess) release();
    return written;
  }
  // For a buffer nothing on the device can still be reading.  No-op when `bytes` fit; otherwise the old buffer is freed
  // first and exactly `bytes` are allocated.  After a failure the buffer is empty and a later call can try again.
  hipError_t reserve_exact(size_t bytes) {
    if (bytes <= bytes_) return hipSuccess;
    release();
    const hipError_t err = hipMalloc(&p_, bytes);
    if (err != hipSuccess) { p_ = nullptr; return err; }
    bytes_ = bytes;
    return hipSuccess;
  }
  // For per-call scratch that queued kernels may still read.  Growth is geometric; the new buffer is allocated first and the
  // old one (its contents are never carried over) goes to `retired` behind an event on `stream`.  Never synchronises.
  hipError_t reserve_retiring(size_t bytes, RetireList &retired, hipStream_t stream) {
    if (bytes <= bytes_) return hipSuccess;
    const size_t cap = std::max(bytes, bytes_ + bytes_ / 2);
    void *fresh = nullptr;
    if (hipError_t err = hipMalloc(&fresh, cap); err != hipSuccess) return err;
    if (p_)
      if (hipError_t err = retired.retire(p_, stream); err != hipSuccess) {
        (void)hipFree(fresh);
        return err;
      }
    p_ = fresh;
    bytes_ = cap;
    return hipSuccess;
  }

 private:
  void *p_ = nullptr;
  size_t bytes_ = 0;
};

// Host-to-device uploads through pinned staging: the host never waits for a stream, and the caller's source may change as
// soon as upload() returns.  One pinned allocation of N equal slots, used in turn; a slot is reused only after the copy that
// read it has completed (its event: N uploads ago, normally long done).  A request larger than a slot waits for the slots in
// flight and reallocates, geometrically.
template <int N>
class PinnedSlots {
 public:
  PinnedSlots() = default;
  PinnedSlots(const PinnedSlots &) = delete;
  PinnedSlots &operator=(const PinnedSlots &) = delete;
  ~PinnedSlots() {
    (void)drain();
    if (pinned_) (void)hipHostFree(pinned_);
  }
  // `a` then `b`, back to back, to `dst`, behind everything already queued on `stream`
  hipError_t upload(void *dst, const void *a, size_t a_bytes, const void *b, size_t b_bytes, hipStream_t stream) {
    const size_t bytes = a_bytes + b_bytes;
    if (bytes > slot_bytes_) {
      if (hipError_t err = drain(); err != hipSuccess) return err;
      const size_t cap = std::max(bytes, slot_bytes_ + slot_bytes_ / 2);
      if (pinned_) (void)hipHostFree(pinned_);
      pinned_ = nullptr;
      slot_bytes_ = 0;
      void *fresh = nullptr;
      if (hipError_t err = hipHostMalloc(&fresh, cap * N, hipHostMallocDefault); err != hipSuccess) return err;
      pinned_ = static_cast<char *>(fresh);
      slot_bytes_ = cap;
    }
    const int slot = next_;
    if (hipError_t err = done_[slot].create(hipEventDisableTiming); err != hipSuccess) return err;
    if (used_[slot]) {
      if (hipError_t err = hipEventSynchronize(done_[slot].get()); err != hipSuccess) return err;
      used_[slot] = false;
    }
    next_ = (next_ + 1) % N;
    char *host = pinned_ + (size_t)slot * slot_bytes_;
    if (a_bytes) std::memcpy(host, a, a_bytes);
    if (b_bytes) std::memcpy(host + a_bytes, b, b_bytes);
    if (hipError_t err = hipMemcpyAsync(dst, host, bytes, hipMemcpyHostToDevice, stream); err != hipSuccess) return err;
    if (hipError_t err = hipEventRecord(done_[slot].get(), stream); err != hipSuccess) return err;
    used_[slot] = true;
    return hipSuccess;
  }
  hipError_t upload(void *dst, const void *src, size_t bytes, hipStream_t stream) { return upload(dst, src, bytes, nullptr, 0, stream); }

 private:
  // wait for every copy still reading a slot
  hipError_t drain() {
    for (int k = 0; k < N; ++k)
      if (used_[k]) {
        if (hipError_t err = hipEventSynchronize(done_[k].get()); err != hipSuccess) return err;
        used_[k] = false;
      }
    return hipSuccess;
  }
  char *pinned_ = nullptr;  // [N][slot_bytes_]
  size_t slot_bytes_ = 0;
  Event done_[N];
  bool used_[N] = {};
  int next_ = 0;
};

// An array of T on the device beside a host copy of what was last sent to it ("the device holds what I last sent"): sync()
// uploads only what differs.  The host copy is taken only after the upload call has succeeded, and anything that could leave
// the two apart (a failed upload, a reallocation, a send() into a sub-range) invalidates it, so the next sync() uploads again.
template <class T>
class Mirrored {
  static_assert(std::is_trivially_copyable<T>::value, "Mirrored compares and copies its elements byte-wise");

 public:
  // room for `count` elements, exactly as DeviceBuffer::reserve_exact (nothing on the device may still be reading)
  hipError_t reserve(size_t count) {
    if (count * sizeof(T) <= buf_.bytes()) return hipSuccess;
    invalidate();
    return buf_.reserve_exact(count * sizeof(T));
  }
  // the first `count` elements <- `src`, behind everything already queued on `stream`, unless that is what they hold
  template <int N>
  hipError_t sync(const T *src, size_t count, PinnedSlots<N> &slots, hipStream_t stream, bool *uploaded = nullptr) {
    if (uploaded) *uploaded = false;
    if (count * sizeof(T) > buf_.bytes()) return hipErrorInvalidValue;
    if (valid_ && held_.size() == count && std::memcmp(held_.data(), src, count * sizeof(T)) == 0) return hipSuccess;
    valid_ = false;
    if (hipError_t err = slots.upload(buf_.get(), src, count * sizeof(T), stream); err != hipSuccess) return err;
    held_.assign(src, src + count);
    valid_ = true;
    if (uploaded) *uploaded = true;
    return hipSuccess;
  }
  // elements [offset, offset + count) <- `src`, always: for slots of the array that are rewritten in turn
  template <int N>
  hipError_t send(size_t offset, const T *src, size_t count, PinnedSlots<N> &slots, hipStream_t stream) {
    invalidate();
    if ((offset + count) * sizeof(T) > buf_.bytes()) return hipErrorInvalidValue;
    return slots.upload(buf_.get() + offset, src, count * sizeof(T), stream);
  }
  void invalidate() { valid_ = false; }
  T *get() const { return buf_.get(); }
  operator T *() const { return get(); }

 private:
  DeviceBuffer<T> buf_;
  std::vector<T> held_;  // what the device holds, while valid_
  bool valid_ = false;
};

// A stream: empty, owned (created non-blocking or with a CU mask: destroyed with the owner), or borrowed (an alias of a
// stream of the caller's: never destroyed).
class Stream {
 public:
  Stream() = default;
  Stream(Stream &&o) noexcept : st_(std::exchange(o.st_, nullptr)), owned_(std::exchange(o.owned_, false)) {}
  Stream &operator=(Stream &&o) noexcept {
    if (this != &o) { reset(); st_ = std::exchange(o.st_, nullptr); owned_ = std::exchange(o.owned_, false); }
    return *this;
  }
  ~Stream() { reset(); }
  // each of the three lets go of what was held; after a failed creation the owner is empty
  hipError_t create() {
    reset();
    return adopt(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
  }
  hipError_t create_with_cu_mask(uint32_t words, const uint32_t *mask) {
    reset();
    return adopt(hipExtStreamCreateWithCUMask(&st_, words, mask));
  }
  void borrow(hipStream_t st) {
    reset();
    st_ = st;
  }
  void reset() {
    if (owned_ && st_) (void)hipStreamDestroy(st_);
    st_ = nullptr;
    owned_ = false;
  }
  hipStream_t get() const { return st_; }
  operator hipStream_t() const { return st_; }

 private:
  hipError_t adopt(hipError_t created) {
    owned_ = created == hipSuccess;
    if (!owned_) st_ = nullptr;
    return created;
  }
  hipStream_t st_ = nullptr;
  bool owned_ = false;
};

// A timing bracket: two events, created at the first begin().  Unused (never begun, or begun and not ended, or a creation
// failed) it reads 0.0 without touching the runtime.
class TimedSpan {
 public:
  hipError_t begin(hipStream_t stream) {
    used_ = false;
    if (hipError_t err = t0_.create(); err != hipSuccess) return err;
    if (hipError_t err = t1_.create(); err != hipSuccess) return err;
    return hipEventRecord(t0_.get(), stream);
  }
  hipError_t end(hipStream_t stream) {
    const hipError_t err = hipEventRecord(t1_.get(), stream);
    used_ = err == hipSuccess;
    return err;
  }
  void clear() { used_ = false; }
  bool used() const { return used_; }
  // waits for the end of the span
  hipError_t elapsed_ms(double *ms) const {
    *ms = 0.0;
    if (!used_) return hipSuccess;
    if (hipError_t err = hipEventSynchronize(t1_.get()); err != hipSuccess) return err;
    float t = 0.0f;
    if (hipError_t err = hipEventElapsedTime(&t, t0_.get(), t1_.get()); err != hipSuccess) return err;
    *ms = t;
    return hipSuccess;
  }

 private:
  Event t0_, t1_;
  bool used_ = false;
};

// Consecutive spans that share their inner events: mark() records the next event of the chain (created when first needed),
// restart() begins a new chain on the same events.
class EventChain {
 public:
  void restart() { marks_ = 0; }
  hipError_t mark(hipStream_t stream) {
    if (marks_ == events_.size()) {
      Event ev;
      if (hipError_t err = ev.create(); err != hipSuccess) return err;
      events_.push_back(std::move(ev));
    }
    if (hipError_t err = hipEventRecord(events_[marks_].get(), stream); err != hipSuccess) return err;
    ++marks_;
    return hipSuccess;
  }
  size_t marks() const { return marks_; }
  hipError_t wait_last() const { return marks_ ? hipEventSynchronize(events_[marks_ - 1].get()) : hipSuccess; }
  // between mark i and mark j, both completed
  hipError_t elapsed(size_t i, size_t j, double *ms) const {
    float t = 0.0f;
    const hipError_t err = hipEventElapsedTime(&t, events_[i].get(), events_[j].get());
    *ms = err == hipSuccess ? (double)t : 0.0;
    return err;
  }

 private:
  std::vector<Event> events_;
  size_t marks_ = 0;
};

// every sample of `rows` rows of `cols`, `stride` apart, is finite
template <class T>
bool check_finite(const T *in, int64_t rows, int64_t cols, int64_t stride) {
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t i = 0; i < cols; ++i)
      if (!std::isfinite(in[r * stride + i])) return false;
  return true;
}

}  // namespace af
