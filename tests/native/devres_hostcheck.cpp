// Host check of the handle-lifetime owners (csrc/mhpc_devres.h) against a fake device: hipMalloc /
// hipFree, the stream and event creations and destructions and hipStreamSynchronize are defined
// here over host malloc, with a failure injectable at the k-th fallible call (an allocation or a
// creation), and every release and synchronise logged in order.  For every k of every sequence:
//  * each owner alone: one release at destruction, none from a moved-from owner, a failed alloc /
//    create leaves the previous object alive (released once, later), ensure() creates once;
//  * a stream set is all or nothing (nine objects, or the handle's own seven; after a failure the
//    set is empty and nothing is alive);
//  * a vector grown to n sets with a failure inside set j holds exactly j complete sets, and a
//    retry completes it without creating the first j again;
//  * grow_and_swap (ensure_knot_arrays' step): a failure at array i frees the i fresh arrays and
//    leaves the seven old ones alive and in place; success frees each old one once, first to last;
//  * a struct with Handle's resource members in Handle's declaration order (mhpc_runtime.cpp: keep
//    the two alike) releases memory before events before streams, no memory before the last
//    synchronise, each set's events before its streams, the main stream last;
//  * at the end of every scenario nothing is alive and no release was bad or double.
// Exit status 0 and "ok" when all hold; the first violated check is printed otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <set>
#include <vector>

#include "../../mhpc_minimal_env_amd/csrc/mhpc_devres.h"

namespace {
struct FakeDevice {
  int calls = 0;     // fallible calls so far (allocations, stream and event creations)
  int fail_at = -1;  // the call (0-based) that fails, -1: none
  int bad = 0;       // releases of something not alive (double or unknown), syncs of a dead stream
  std::map<void*, size_t> mem;  // live allocations with their sizes
  std::set<void*> streams, events;
  struct Rel {
    char kind;  // 'F'ree, 'E'vent destroyed, 'S'tream destroyed, s'Y'nchronise
    void* p;
  };
  std::vector<Rel> log;
  bool step() { return calls++ != fail_at; }
  size_t live() const { return mem.size() + streams.size() + events.size(); }
  int count(char kind) const {
    int n = 0;
    for (const Rel& r : log) n += r.kind == kind;
    return n;
  }
} dev;
int failures = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      ++failures;                           \
      printf("FAILED %s: ", #cond);         \
      printf(__VA_ARGS__);                  \
      printf("\n");                         \
    }                                       \
  } while (0)

void reset(int fail_at) {
  dev = FakeDevice();
  dev.fail_at = fail_at;
}
// the end of every scenario
void totals(const char* what, int k) {
  CHECK(dev.live() == 0 && dev.bad == 0, "%s fail_at %d: %zu alive, %d bad releases", what, k, dev.live(), dev.bad);
}
}  // namespace

hipError_t hipMalloc(void** p, size_t bytes) {
  if (!dev.step()) return hipErrorOutOfMemory;  // (*p untouched, as the runtime leaves it)
  *p = malloc(bytes ? bytes : 1);
  dev.mem[*p] = bytes;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  dev.log.push_back({'F', p});
  if (!dev.mem.erase(p)) return ++dev.bad, hipErrorInvalidValue;
  free(p);
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
  if (flags != hipStreamNonBlocking) ++dev.bad;
  if (!dev.step()) return hipErrorOutOfMemory;
  *s = (hipStream_t)malloc(1);
  dev.streams.insert(*s);
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  dev.log.push_back({'S', s});
  if (!dev.streams.erase(s)) return ++dev.bad, hipErrorInvalidHandle;
  free(s);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
  dev.log.push_back({'Y', s});
  if (!dev.streams.count(s)) return ++dev.bad, hipErrorInvalidHandle;  // (null included)
  return hipSuccess;
}
static hipError_t event_create(hipEvent_t* e) {
  if (!dev.step()) return hipErrorOutOfMemory;
  *e = (hipEvent_t)malloc(1);
  dev.events.insert(*e);
  return hipSuccess;
}
int timed_events = 0;
hipError_t hipEventCreate(hipEvent_t* e) {
  ++timed_events;
  return event_create(e);
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  if (flags != hipEventDisableTiming) ++dev.bad;
  return event_create(e);
}
hipError_t hipEventDestroy(hipEvent_t e) {
  dev.log.push_back({'E', e});
  if (!dev.events.erase(e)) return ++dev.bad, hipErrorInvalidHandle;
  free(e);
  return hipSuccess;
}

namespace {
// ---- each owner alone: create, replace, move.  Three fallible calls; X is Stream or Event.
hipError_t make(DevArray<double>& a, int n) { return a.alloc(n); }
hipError_t make(Stream& s, int) { return s.create(); }
hipError_t make(Event& e, int n) { return e.create(n & 1 ? EV_TIMING : EV_ORDER); }
void* raw(const DevArray<double>& a) { return a.get(); }
void* raw(const Stream& s) { return (hipStream_t)s; }
void* raw(const Event& e) { return (hipEvent_t)e; }

template <class X>
int owner_alone(const char* what, int k) {
  reset(k);
  {
    X a;
    CHECK(raw(a) == nullptr && dev.live() == 0, "%s: a new owner is not empty", what);
    const hipError_t e0 = make(a, 3);  // call 0
    CHECK((e0 == hipSuccess) == (k != 0), "%s fail_at %d: first creation", what, k);
    CHECK(dev.live() == (k != 0) && (raw(a) != nullptr) == (k != 0), "%s fail_at %d: after the first creation", what, k);
    void* const first = raw(a);
    const hipError_t e1 = make(a, 8);  // call 1: replaces; a failure keeps the first
    CHECK((e1 == hipSuccess) == (k != 1), "%s fail_at %d: second creation", what, k);
    if (k == 1) CHECK(raw(a) == first && dev.live() == 1 && dev.log.empty(), "%s: a failed creation touched the owner", what);
    if (k != 1 && first) CHECK(dev.log.size() == 1 && dev.log[0].p == first, "%s fail_at %d: the replaced object is released once", what, k);
    CHECK(dev.live() == (raw(a) != nullptr), "%s fail_at %d: alive after the second creation", what, k);
    void* const held = raw(a);
    const size_t before = dev.log.size();
    X b(std::move(a));
    CHECK(raw(a) == nullptr && raw(b) == held, "%s fail_at %d: move construction", what, k);
    X c;
    const hipError_t e2 = make(c, 5);  // call 2
    CHECK((e2 == hipSuccess) == (k != 2), "%s fail_at %d: third creation", what, k);
    void* const cs = raw(c);
    c = std::move(b);  // c's own object goes with the moved-from b
    CHECK(raw(c) == held, "%s fail_at %d: move assignment", what, k);
    { X gone(std::move(b)); }
    CHECK(dev.log.size() == before + (cs != nullptr), "%s fail_at %d: the moved-from owners released %zu", what, k,
          dev.log.size() - before);
    CHECK(dev.live() == (held != nullptr), "%s fail_at %d: alive before destruction", what, k);
  }
  totals(what, k);
  return dev.calls;
}

void ensure_once() {
  reset(-1);
  timed_events = 0;
  {
    Stream s;
    Event e, t;
    CHECK(s.ensure() == hipSuccess && e.ensure() == hipSuccess && t.ensure(EV_TIMING) == hipSuccess, "ensure");
    void *s0 = raw(s), *e0 = raw(e), *t0 = raw(t);
    CHECK(s.ensure() == hipSuccess && e.ensure() == hipSuccess && t.ensure(EV_TIMING) == hipSuccess, "ensure again");
    CHECK(dev.calls == 3 && raw(s) == s0 && raw(e) == e0 && raw(t) == t0, "ensure() created again: %d calls", dev.calls);
    CHECK(timed_events == 1, "%d timing events of 1", timed_events);
  }
  totals("ensure", -1);
  for (int k = 0; k < 3; ++k) {  // a failed ensure() leaves an empty owner that the next one fills
    reset(k);
    {
      Stream s;
      Event e, t;
      const hipError_t r[3] = {s.ensure(), e.ensure(), t.ensure(EV_TIMING)};
      for (int i = 0; i < 3; ++i) CHECK((r[i] == hipSuccess) == (i != k), "ensure %d fail_at %d", i, k);
      CHECK(dev.live() == 2, "ensure fail_at %d: %zu alive", k, dev.live());
      CHECK(s.ensure() == hipSuccess && e.ensure() == hipSuccess && t.ensure(EV_TIMING) == hipSuccess &&
                dev.live() == 3 && dev.calls == 4,
            "ensure fail_at %d: the retry", k);
    }
    totals("ensure", k);
  }
}

// ---- stream sets
bool empty(const StreamSet& q) {
  return !q.s1 && !q.s2 && !q.s3 && !q.fork && !q.join && !q.pfork && !q.pjoin && !q.gate && !q.done;
}
bool complete(const StreamSet& q, bool sub) {
  return q.s1 && q.s2 && q.s3 && q.fork && q.join && q.pfork && q.pjoin && !q.gate == !sub && !q.done == !sub;
}
int stream_set(bool sub, int k) {
  const int n = sub ? 9 : 7;
  reset(k);
  {
    StreamSet q;
    const hipError_t e = q.create(sub);
    if (k < 0 || k >= n) {
      CHECK(e == hipSuccess && complete(q, sub) && dev.live() == (size_t)n, "set of %d: %zu alive", n, dev.live());
      CHECK(dev.streams.size() == 3 && q.sync() == hipSuccess && dev.count('Y') == 3, "set of %d: sync", n);
    } else {
      CHECK(e != hipSuccess && empty(q) && dev.live() == 0, "set of %d fail_at %d: %zu alive after the failure", n, k,
            dev.live());
      CHECK(dev.calls == k + 1, "set of %d fail_at %d: %d creations", n, k, dev.calls);
      CHECK(q.sync() == hipSuccess && dev.count('Y') == 0, "an empty set synchronised something");
    }
  }
  CHECK((int)dev.log.size() - dev.count('Y') == (k < 0 ? n : k), "set of %d fail_at %d: %zu releases", n, k, dev.log.size());
  totals("stream set", k);
  return dev.calls;
}

// ---- the rule of ensure_sub_streams
void grow_sets(int n, int k) {
  reset(k);
  {
    std::vector<StreamSet> v;
    const hipError_t e = grow_stream_sets(v, n);
    const int j = k < 0 ? n : k / 9;
    CHECK((e == hipSuccess) == (k < 0) && (int)v.size() == j && dev.live() == (size_t)9 * j,
          "%d sets fail_at %d: %zu sets, %zu alive", n, k, v.size(), dev.live());
    std::vector<void*> s1;
    for (const StreamSet& q : v) {
      CHECK(complete(q, true), "%d sets fail_at %d: an incomplete set in the vector", n, k);
      s1.push_back(raw(q.s1));
    }
    const int before = dev.calls;
    dev.fail_at = -1;
    CHECK(grow_stream_sets(v, n) == hipSuccess && (int)v.size() == n && dev.live() == (size_t)9 * n,
          "%d sets fail_at %d: the retry", n, k);
    CHECK(dev.calls - before == 9 * (n - j), "%d sets fail_at %d: the retry made %d creations", n, k, dev.calls - before);
    for (int i = 0; i < j; ++i) CHECK(raw(v[i].s1) == s1[i], "%d sets fail_at %d: set %d was created again", n, k, i);
    for (const StreamSet& q : v) CHECK(complete(q, true), "%d sets fail_at %d: incomplete after the retry", n, k);
  }
  totals("grown sets", k);
}

// ---- ensure_knot_arrays' step
void knot_arrays(int k) {  // k: the fresh array (0..6) whose allocation fails, -1: none
  reset(-1);
  {
    DevArray<float> a[7];
    DevArray<float>* const arr[] = {&a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6]};
    const size_t small[] = {30, 1, 56, 4, 14, 9, 10}, big[] = {60, 2, 112, 8, 28, 18, 20};
    CHECK(grow_and_swap(arr, small) == hipSuccess && dev.live() == 7 && dev.log.empty(), "the first arrays");
    void* old[7];
    for (int i = 0; i < 7; ++i) {
      old[i] = a[i].get();
      CHECK(dev.mem[old[i]] == small[i] * sizeof(float), "array %d: %zu bytes", i, dev.mem[old[i]]);
    }
    dev.fail_at = k < 0 ? -1 : dev.calls + k;
    const hipError_t e = grow_and_swap(arr, big);
    CHECK((e == hipSuccess) == (k < 0), "knot arrays fail_at %d", k);
    CHECK(dev.live() == 7 && dev.count('F') == (k < 0 ? 7 : k), "knot arrays fail_at %d: %zu alive, %d frees", k,
          dev.live(), dev.count('F'));
    for (int i = 0; i < 7; ++i)
      if (k < 0) {
        CHECK(dev.log[i].p == old[i] && dev.mem.count(a[i].get()) && dev.mem[a[i].get()] == big[i] * sizeof(float),
              "array %d after the swap", i);
      } else {
        CHECK(a[i].get() == old[i] && dev.mem.count(old[i]) && dev.mem[old[i]] == small[i] * sizeof(float),
              "knot arrays fail_at %d: array %d changed", k, i);
      }
  }
  totals("knot arrays", k);
}

// ---- destruction order: Handle's resource members, in Handle's declaration order
struct HandleResources {
  StreamSet main;
  Event evstart;
  std::vector<StreamSet> subs;
  Event ev0, ev1;
  std::vector<Event> evpool;
  Event evctl, evt0, evt1;
  DevArray<int> dstep, dsplit;
  DevArray<float> store;
  DevArray<unsigned long long> dcnt;
  struct Arrays {
    DevArray<int> oid;
    DevArray<char> opt;
    DevArray<char> cmd;
    DevArray<int> lid, gidx;
    DevArray<char> grp;
    DevArray<char> carry;
    DevArray<float> out;
    DevArray<char> st;
    DevArray<float> x0, px, par, G, du, K, refpos, traj;
  } own;
};
// Everything a handle ever creates, in the order of its calls; stops at the first failure, as
// mhpc_create does before it destroys the handle.
hipError_t populate(HandleResources& h) {
  HandleResources::Arrays& a = h.own;
  hipError_t e = hipSuccess;
  auto alloc = [&](auto& arr, size_t n) {
    if (e == hipSuccess) e = arr.alloc(n);
  };
  alloc(a.px, 8), alloc(a.x0, 8), alloc(a.st, 8), alloc(a.carry, 8), alloc(h.dcnt, 8), alloc(a.grp, 8);
  alloc(a.gidx, 8), alloc(a.lid, 8), alloc(h.dsplit, 8), alloc(a.opt, 8), alloc(a.oid, 8);
  if (e == hipSuccess) e = h.main.create(false);
  if (e == hipSuccess) e = h.ev0.create(EV_TIMING);
  if (e == hipSuccess) e = h.ev1.create(EV_TIMING);
  DevArray<float>* const arr[] = {&a.traj, &a.refpos, &a.K, &a.du, &a.G, &a.par, &a.out};
  const size_t count[] = {8, 8, 8, 8, 8, 8, 8};
  if (e == hipSuccess) e = grow_and_swap(arr, count);
  alloc(a.cmd, 8);
  if (e == hipSuccess) e = h.evstart.ensure();
  if (e == hipSuccess) e = grow_stream_sets(h.subs, 2);
  for (int i = 0; i < 4 && e == hipSuccess; ++i) {
    Event ev;
    if ((e = ev.create(EV_TIMING)) == hipSuccess) h.evpool.push_back(std::move(ev));
  }
  alloc(h.store, 8);
  if (e == hipSuccess) e = h.evt0.ensure(EV_TIMING);
  if (e == hipSuccess) e = h.evt1.ensure(EV_TIMING);
  alloc(h.dstep, 8);
  if (e == hipSuccess) e = h.evctl.ensure();
  return e;
}
int destruction_order(int k) {
  reset(k);
  void *main_s1 = nullptr, *traj = nullptr, *dstep = nullptr;
  std::map<void*, int> set_of;  // stream or event -> its set (0: main, 1..: subs)
  {
    HandleResources h;
    const hipError_t e = populate(h);
    CHECK((e == hipSuccess) == (k < 0), "populate fail_at %d", k);
    main_s1 = raw(h.main.s1), traj = h.own.traj.get(), dstep = h.dstep.get();
    int i = 0;
    auto note = [&](const StreamSet& q) {
      for (void* p : {raw(q.s1), raw(q.s2), raw(q.s3), raw(q.fork), raw(q.join), raw(q.pfork), raw(q.pjoin),
                      raw(q.gate), raw(q.done)})
        if (p) set_of[p] = i;
      ++i;
    };
    note(h.main);
    for (const StreamSet& q : h.subs) note(q);
    // mhpc_destroy: every stream of the handle drained, then delete
    (void)h.main.sync();
    for (const StreamSet& q : h.subs) (void)q.sync();
  }
  totals("handle", k);
  if (k >= 0) return dev.calls;
  const std::vector<FakeDevice::Rel>& log = dev.log;
  CHECK(dev.count('Y') == 9 && dev.count('F') == 21 && dev.count('S') == 9 && dev.count('E') == 4 + 12 + 1 + 2 + 4 + 3,
        "handle: %d syncs, %d frees, %d streams, %d events", dev.count('Y'), dev.count('F'), dev.count('S'),
        dev.count('E'));
  size_t last_sync = 0, first_free = log.size(), last_free = 0, first_obj = log.size();
  for (size_t i = 0; i < log.size(); ++i) {
    if (log[i].kind == 'Y') last_sync = i;
    if (log[i].kind == 'F') first_free = std::min(first_free, i), last_free = i;
    if (log[i].kind == 'E' || log[i].kind == 'S') first_obj = std::min(first_obj, i);
  }
  CHECK(last_sync < first_free, "handle: memory freed before the last synchronise");
  CHECK(last_free < first_obj, "handle: an event or stream destroyed before the last free");
  CHECK(log[first_free].p == traj && log[last_free].p == dstep, "handle: the arrays' order of release changed");
  CHECK(log.back().kind == 'S' && log.back().p == main_s1, "handle: the main stream is not the last to go");
  // each set: its events before its streams; and every event outside the sets (recorded on the
  // main stream, or on a caller's) before the main set's streams
  std::map<int, size_t> first_stream;
  for (size_t i = log.size(); i-- > 0;)
    if (log[i].kind == 'S') first_stream[set_of[log[i].p]] = i;
  for (size_t i = 0; i < log.size(); ++i)
    if (log[i].kind == 'E') {
      const int s = set_of.count(log[i].p) ? set_of[log[i].p] : 0;
      CHECK(i < first_stream[s], "handle: an event of set %d destroyed after a stream of the set", s);
    }
  return dev.calls;
}
}  // namespace

int main() {
  for (int k = -1; k < 3; ++k) {
    CHECK(owner_alone<DevArray<double>>("array", k) == 3, "array: fallible calls");
    CHECK(owner_alone<Stream>("stream", k) == 3, "stream: fallible calls");
    CHECK(owner_alone<Event>("event", k) == 3, "event: fallible calls");
  }
  ensure_once();
  CHECK(stream_set(true, -1) == 9 && stream_set(false, -1) == 7, "creations of a stream set");
  for (int k = 0; k < 9; ++k) stream_set(true, k);
  for (int k = 0; k < 7; ++k) stream_set(false, k);
  for (int k = -1; k < 27; ++k) grow_sets(3, k);
  for (int k = -1; k < 7; ++k) knot_arrays(k);
  const int n = destruction_order(-1);
  CHECK(n == 11 + 7 + 2 + 7 + 1 + 1 + 18 + 4 + 1 + 2 + 1 + 1, "%d fallible calls in a handle's life", n);
  for (int k = 0; k < n; ++k) destruction_order(k);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
