// Device temporaries of one call: the arrays a C-ABI entry point allocates, fills from the
// caller's double arrays, hands to a launch, reads back and frees.  One owner for all of it:
//   DevTemp<real> t(stream);              // stream null: blocking copies on the null stream
//   real* dx = t.in(x, n);                // device array <- (real)x[i]  (or a staged vector)
//   real* dy = t.out(y, m);               // device array -> y[i] = (double)dy[i] at fetch()
//   if (t.e == hipSuccess) t.e = launch(dx, dy, ...);
//   if (t.fetch() != hipSuccess) ...      // every allocation is freed by the destructor
// The error is sticky: after the first failure no call touches the device again (but the
// destructor's frees), pointers returned later are null, and fetch() writes no caller array --
// a failed call leaves every output as it was.  Conversion is static_cast both ways.
// Every allocation carries 8 spare bytes, as the model hooks' temporaries always did.
#pragma once
#include <hip/hip_runtime_api.h>

#include <stddef.h>

#include <utility>
#include <vector>

template <typename T>
class DevTemp {
 public:
  hipError_t e = hipSuccess;

  explicit DevTemp(hipStream_t stream = nullptr) : stream_(stream) {}
  DevTemp(const DevTemp&) = delete;
  DevTemp& operator=(const DevTemp&) = delete;
  ~DevTemp() {
    for (void* p : ptrs_) (void)hipFree(p);
  }

  T* alloc(size_t n) { return (T*)alloc_bytes(n * sizeof(T)); }
  T* in(const double* host, size_t n) { return in(std::vector<T>(host, host + n)); }
  // a host array the caller converted (and padded) itself; kept as long as *this, since an
  // asynchronous copy reads it
  T* in(std::vector<T>&& host) {
    if (e != hipSuccess) return nullptr;
    tin_.push_back(std::move(host));
    return (T*)upload(tin_.back().data(), tin_.back().size() * sizeof(T));
  }
  double* in_double(std::vector<double>&& host) {  // doubles for the device as they are
    if (e != hipSuccess) return nullptr;
    din_.push_back(std::move(host));
    return (double*)upload(din_.back().data(), din_.back().size() * sizeof(double));
  }
  // host null: staged only (staged())
  T* out(double* host, size_t n) {
    T* p = alloc(n);
    if (e == hipSuccess) outs_.push_back({p, host, n, std::vector<T>(n)});
    return p;
  }
  // Every out() array to its host staging copy, then the stream drained; no caller array yet.
  void stage() {
    for (Out& o : outs_) copy(o.staged.data(), o.dev, o.n * sizeof(T), hipMemcpyDeviceToHost);
    if (e == hipSuccess && stream_) e = hipStreamSynchronize(stream_);
    staged_ = e == hipSuccess;
  }
  // stage() unless done, then every out() array with a host array converted into it.
  hipError_t fetch() {
    if (!staged_) stage();
    if (e != hipSuccess) return e;
    for (const Out& o : outs_)
      for (size_t i = 0; o.host && i < o.n; ++i) o.host[i] = static_cast<double>(o.staged[i]);
    return e;
  }
  // The staged host copy of out() array dev, valid after a successful stage() / fetch().
  const T* staged(const T* dev) const {
    for (const Out& o : outs_)
      if (o.dev == dev) return o.staged.data();
    return nullptr;
  }

 private:
  struct Out {
    T* dev;
    double* host;
    size_t n;
    std::vector<T> staged;
  };
  void* alloc_bytes(size_t bytes) {
    void* p = nullptr;
    if (e == hipSuccess) e = hipMalloc(&p, bytes + 8);
    if (e != hipSuccess) return nullptr;
    ptrs_.push_back(p);
    return p;
  }
  void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (e != hipSuccess) return;
    e = stream_ ? hipMemcpyAsync(dst, src, bytes, kind, stream_) : hipMemcpy(dst, src, bytes, kind);
  }
  void* upload(const void* host, size_t bytes) {
    void* p = alloc_bytes(bytes);
    copy(p, host, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? p : nullptr;
  }

  hipStream_t stream_;
  bool staged_ = false;
  std::vector<void*> ptrs_;
  std::vector<Out> outs_;
  std::vector<std::vector<T>> tin_;
  std::vector<std::vector<double>> din_;
};
