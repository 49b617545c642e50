// A fake HIP runtime for the stand-alone host tests of this directory (they are not linked against the real one): allocations
// over malloc, one queue for every stream, whose copies and event records run when the test drains it, a synchronous copy,
// live sets of what was created, and a switch that fails the k-th fallible call.  Include it once, in the file with main().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

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
std::set<hipStream_t> streams;  // live streams the fake created
long stream_destroys = 0;
std::vector<size_t> alloc_log;  // bytes of every device allocation, in order
long device_frees = 0;          // device allocations freed
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
  alloc_log.clear();
  device_frees = 0;
  calls = fallible = fail_at = pinned_allocs = blocking_waits = stream_destroys = 0;
  query_fails_once = false;
  sticky = hipSuccess;
}
bool nothing_live() { return device.empty() && pinned.empty() && events.empty() && streams.empty(); }
hipError_t create_stream(hipStream_t *st) {
  ++calls;
  if (inject()) return hipErrorOutOfMemory;
  *st = reinterpret_cast<hipStream_t>(new char);
  streams.insert(*st);
  return hipSuccess;
}
}  // namespace fake

hipError_t hipMalloc(void **p, size_t n) {
  ++fake::calls;
  if (fake::inject()) return hipErrorOutOfMemory;
  *p = std::malloc(n ? n : 1);
  fake::device[*p] = n;
  fake::alloc_log.push_back(n);
  return hipSuccess;
}
hipError_t hipFree(void *p) {
  ++fake::calls;
  if (!p) return hipSuccess;
  if (!fake::device.erase(p)) { std::fprintf(stderr, "hipFree of a pointer that is not live\n"); std::abort(); }
  std::free(p);
  ++fake::device_frees;
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
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) {  // behind everything queued, then at once
  ++fake::calls;
  if (fake::inject()) return hipErrorUnknown;
  fake::drain_all();
  if (bytes) std::memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *st, unsigned) { return fake::create_stream(st); }
hipError_t hipExtStreamCreateWithCUMask(hipStream_t *st, uint32_t, const uint32_t *) { return fake::create_stream(st); }
hipError_t hipStreamDestroy(hipStream_t st) {
  ++fake::calls;
  ++fake::stream_destroys;
  if (!fake::streams.erase(st)) { std::fprintf(stderr, "hipStreamDestroy of a stream that is not live\n"); std::abort(); }
  delete reinterpret_cast<char *>(st);
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
