// Device resources that live as long as a handle (or a snapshot's staging): move-only owners of
// one device array, one stream, one event, and of the streams and events one run of the solve
// schedule uses.  Creation returns the hipError_t and, on a failure, leaves the owner as it was;
// the destructor releases.  (Per-call temporaries: mhpc_devtemp.h.)  Host code only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <stddef.h>

#include <utility>
#include <vector>

template <typename T>
class DevArray {
 public:
  DevArray() = default;
  DevArray(DevArray&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevArray& operator=(DevArray&& o) noexcept { return swap(o), *this; }  // (o frees the previous one)
  ~DevArray() { reset(); }
  // A fresh array of n elements; the previous one is freed after that, and stays on a failure.
  hipError_t alloc(size_t n) {
    DevArray fresh;
    const hipError_t e = hipMalloc((void**)&fresh.p_, n * sizeof(T));
    if (e == hipSuccess) swap(fresh);
    return e;
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  T* get() const { return p_; }
  void swap(DevArray& o) { std::swap(p_, o.p_); }

 private:
  T* p_ = nullptr;
};

// n fresh arrays of count[i] elements, swapped into *arr[i] once all of them exist (the previous
// arrays are then freed, first to last).  On a failure the fresh ones are freed and every *arr[i]
// is what it was.
template <typename T, size_t N>
hipError_t grow_and_swap(DevArray<T>* const (&arr)[N], const size_t (&count)[N]) {
  DevArray<T> fresh[N];
  for (size_t i = 0; i < N; ++i)
    if (hipError_t e = fresh[i].alloc(count[i])) return e;
  for (size_t i = 0; i < N; ++i) {
    arr[i]->swap(fresh[i]);
    fresh[i].reset();
  }
  return hipSuccess;
}

// A non-blocking stream and an event.  Each converts to its raw handle, so an owner stands
// wherever the HIP API takes one; create() on a live owner replaces it, and keeps it on a failure.
class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept { return std::swap(s_, o.s_), *this; }
  ~Stream() {
    if (s_) (void)hipStreamDestroy(s_);
  }
  hipError_t create() {
    Stream fresh;
    const hipError_t e = hipStreamCreateWithFlags(&fresh.s_, hipStreamNonBlocking);
    if (e == hipSuccess) std::swap(s_, fresh.s_);
    return e;
  }
  hipError_t ensure() { return s_ ? hipSuccess : create(); }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

enum EventKind { EV_ORDER, EV_TIMING };  // hipEventDisableTiming, or an event that measures
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : ev_(o.ev_) { o.ev_ = nullptr; }
  Event& operator=(Event&& o) noexcept { return std::swap(ev_, o.ev_), *this; }
  ~Event() {
    if (ev_) (void)hipEventDestroy(ev_);
  }
  hipError_t create(EventKind kind = EV_ORDER) {
    Event fresh;
    const hipError_t e = kind == EV_TIMING ? hipEventCreate(&fresh.ev_)
                                           : hipEventCreateWithFlags(&fresh.ev_, hipEventDisableTiming);
    if (e == hipSuccess) std::swap(ev_, fresh.ev_);
    return e;
  }
  hipError_t ensure(EventKind kind = EV_ORDER) { return ev_ ? hipSuccess : create(kind); }
  operator hipEvent_t() const { return ev_; }

 private:
  hipEvent_t ev_ = nullptr;
};

// The streams and events of one run of the solve schedule: the chain's stream, the partials' two
// (s3: their second group) with the events that fork them off and join them back, and for a
// sub-batch the gate to the next block and the end of its own.  Declared streams first: the
// events go before the streams they were recorded on, s1 last.
struct StreamSet {
  Stream s1, s2, s3;
  Event fork, join, pfork, pjoin, gate, done;
  // All of the set or nothing: on a failure *this stays empty and nothing stays alive.  sub: a
  // sub-batch's set of nine; otherwise a handle's own seven (no gate, no done).  Each in the order
  // its creations always had.
  hipError_t create(bool sub) {
    StreamSet t;
    hipError_t e = t.s1.create();
    auto then = [&e](auto& x) {
      if (e == hipSuccess) e = x.create();
    };
    then(t.s2);
    if (!sub) then(t.fork), then(t.join);
    then(t.s3);
    then(t.pfork), then(t.pjoin);
    if (sub) then(t.fork), then(t.join), then(t.gate), then(t.done);
    if (e == hipSuccess) *this = std::move(t);
    return e;
  }
  // Every stream of the set drained (all three are tried); the first error.
  hipError_t sync() const {
    hipError_t e = hipSuccess;
    for (hipStream_t q : {(hipStream_t)s1, (hipStream_t)s2, (hipStream_t)s3}) {
      const hipError_t e1 = q ? hipStreamSynchronize(q) : hipSuccess;
      if (e == hipSuccess) e = e1;
    }
    return e;
  }
};

// v grown to n complete sub-batch sets: a set is appended only once all of it exists, so after a
// failure v holds the complete ones and a retry goes on from there.
inline hipError_t grow_stream_sets(std::vector<StreamSet>& v, size_t n) {
  while (v.size() < n) {
    StreamSet s;
    if (hipError_t e = s.create(true)) return e;
    v.push_back(std::move(s));
  }
  return hipSuccess;
}
