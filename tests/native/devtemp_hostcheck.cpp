// Host check of DevTemp (csrc/mhpc_devtemp.h) against a fake device: hipMalloc / hipFree /
// hipMemcpy(Async) / hipStreamSynchronize are defined here over host malloc, with a failure
// injectable at the k-th allocation, copy or synchronise, so the helper links to them and not
// to the HIP runtime.  Checked for float and double elements, with and without a stream:
//  * success: values round-trip as static_cast gives them, frees equal allocations;
//  * a failure at every point of a 3-input / 3-output sequence (lengths 1, 5, 196; plus an
//    unconverted and a caller-staged input, and one output without a host array): the error is
//    sticky, no later fake-device call happens, no output array changes, and every
//    successful allocation is freed exactly once.
// Exit status 0 and "ok" when all hold; the first violated check is printed otherwise.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <set>

#include "../../mhpc_minimal_env_amd/csrc/mhpc_devtemp.h"

namespace {
struct FakeDevice {
  int calls = 0;        // fallible calls so far (allocations, copies, synchronises)
  int fail_at = -1;     // the call (0-based) that fails, -1: none
  int after_fail = 0;   // fallible calls after the failed one
  int allocs = 0, frees = 0, bad_frees = 0;
  std::set<void*> live;
  bool step() {  // false: this call fails
    if (fail_at >= 0 && calls > fail_at) ++after_fail;
    return calls++ != fail_at;
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
}  // namespace

hipError_t hipMalloc(void** p, size_t bytes) {
  *p = nullptr;
  if (!dev.step()) return hipErrorOutOfMemory;
  *p = malloc(bytes);
  memset(*p, 0xAB, bytes);
  dev.live.insert(*p);
  ++dev.allocs;
  return hipSuccess;
}
hipError_t hipFree(void* p) {  // not fallible: the destructor's frees always run
  if (!dev.live.erase(p)) {
    ++dev.bad_frees;
    return hipErrorInvalidValue;
  }
  free(p);
  ++dev.frees;
  return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  if (!dev.step()) return hipErrorInvalidValue;
  memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
  return hipMemcpy(dst, src, bytes, kind);
}
hipError_t hipStreamSynchronize(hipStream_t) {
  return dev.step() ? hipSuccess : hipErrorUnknown;
}

namespace {
constexpr size_t LEN[3] = {1, 5, 196};
constexpr double SENTINEL = -77.25;

// in[j][i]: a value float cannot hold, a signed zero and a float denormal among ordinary ones
double value(int j, size_t i) {
  switch ((i + j) % 5) {
    case 0: return 0.1 + (double)i;  // not representable in float
    case 1: return -0.0;
    case 2: return 1e-40;            // denormal as a float
    case 3: return -(double)(i + 1) / 3.0;
    default: return (double)std::numeric_limits<float>::max();
  }
}
bool same(double a, double b) { return a == b && signbit(a) == signbit(b); }

// 3 inputs and 3 outputs; the "kernel" copies input j to output j on the fake device.  Returns
// the fallible calls a successful sequence makes.
template <typename T>
int sequence(hipStream_t stream, int fail_at) {
  dev = FakeDevice();
  dev.fail_at = fail_at;
  double in[3][196], out[3][196], raw[196];
  for (int j = 0; j < 3; ++j)
    for (size_t i = 0; i < 196; ++i) {
      in[j][i] = value(j, i);
      out[j][i] = SENTINEL;
    }
  const char* what = sizeof(T) == 4 ? "float" : "double";
  {
    DevTemp<T> t(stream);
    T *din[3], *dout[3];
    for (int j = 0; j < 3; ++j) din[j] = t.in(in[j], LEN[j]);
    const double* draw = t.in_double(std::vector<double>(in[2], in[2] + LEN[2]));
    const T* dstaged = t.in(std::vector<T>(LEN[1], T(3)));
    for (int j = 0; j < 3; ++j) dout[j] = t.out(j == 1 ? nullptr : out[j], LEN[j]);
    const hipError_t first = t.e;
    if (t.e == hipSuccess) {
      for (int j = 0; j < 3; ++j) memcpy(dout[j], din[j], LEN[j] * sizeof(T));
      memcpy(raw, draw, sizeof raw);
      CHECK(dstaged[0] == T(3) && dstaged[LEN[1] - 1] == T(3), "%s: staged input not uploaded", what);
    }
    const hipError_t got = t.fetch();
    CHECK(got == t.e, "%s fail_at %d: fetch() returns the sticky error", what, fail_at);
    if (fail_at < 0) {
      CHECK(got == hipSuccess, "%s: error %d without an injected failure", what, (int)got);
      for (int j = 0; j < 3; ++j)
        for (size_t i = 0; i < LEN[j]; ++i) {
          const double want = static_cast<double>(static_cast<T>(in[j][i]));
          const double have = j == 1 ? static_cast<double>(t.staged(dout[1])[i]) : out[j][i];
          CHECK(same(have, want), "%s out %d[%zu]: %a, expected %a", what, j, i, have, want);
        }
      for (size_t i = 0; i < 196; ++i)
        CHECK(same(raw[i], in[2][i]), "%s in_double[%zu] was converted", what, i);
      for (int j = 0; j < 3; ++j)
        for (size_t i = LEN[j]; i < 196; ++i)
          CHECK(same(out[j][i], SENTINEL), "%s out %d written past its length", what, j);
    } else {
      CHECK(got != hipSuccess, "%s fail_at %d: the failure was lost", what, fail_at);
      CHECK(first == hipSuccess || first == got, "%s fail_at %d: the error changed", what, fail_at);
      CHECK(t.fetch() == got, "%s fail_at %d: a second fetch() changed the error", what, fail_at);
      for (int j = 0; j < 3; ++j)
        for (size_t i = 0; i < 196; ++i)
          CHECK(same(out[j][i], SENTINEL), "%s fail_at %d: out %d[%zu] written", what, fail_at, j, i);
      CHECK(t.in(in[0], 1) == nullptr && t.alloc(4) == nullptr && t.out(out[0], 1) == nullptr,
            "%s fail_at %d: a pointer handed out after the error", what, fail_at);
    }
    CHECK(dev.after_fail == 0, "%s fail_at %d: %d device calls after the failure", what, fail_at,
          dev.after_fail);
    CHECK(dev.frees == 0, "%s fail_at %d: freed before destruction", what, fail_at);
  }
  CHECK(dev.frees == dev.allocs && dev.live.empty() && dev.bad_frees == 0,
        "%s fail_at %d: %d allocations, %d frees, %d bad frees", what, fail_at, dev.allocs,
        dev.frees, dev.bad_frees);
  return dev.calls;
}

template <typename T>
void check(hipStream_t stream) {
  // 8 allocations + 5 uploads, 3 downloads, and the synchronise of a stream
  const int n = sequence<T>(stream, -1);
  CHECK(n == (stream ? 17 : 16), "%d fallible calls in a successful sequence", n);
  for (int k = 0; k < n; ++k) sequence<T>(stream, k);
}
}  // namespace

int main() {
  int dummy;
  hipStream_t stream = (hipStream_t)&dummy;  // never dereferenced by the fake device
  check<float>(nullptr);
  check<float>(stream);
  check<double>(nullptr);
  check<double>(stream);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
