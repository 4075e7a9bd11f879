// device_buffers.h — who frees the host side's device objects: device_buffer<T> (hipMalloc / hipFree) and pinned_buffer<T> (hipHostMalloc /
// hipHostFree), move-only owners of `count` elements of T; hip_stream and hip_event; and hip_steps, a list of allocations (and the HIP
// calls between them) that stops at the first error. An object made of these is freed by `delete`; a grow is reset, allocate, set the
// capacity. Nothing here selects a device: the caller has. The only file of csrc that names a HIP call that frees or destroys.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <utility>
#include <vector>

// An object of the C APIs that owns such buffers has a destructor, and its type's name is global (the public headers declare it): the
// type is marked SS_HIDDEN so that the library exports nothing it did not export while the objects were freed by hand.
#define SS_HIDDEN __attribute__((visibility("hidden")))

namespace ss {
namespace {  // (each translation unit, specscan.hip and channelizer.hip, has its own: nothing of it is exported)

template <class T, bool Pinned>
class hip_buffer {
 public:
  hip_buffer() = default;
  hip_buffer(hip_buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  hip_buffer& operator=(hip_buffer&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
    }
    return *this;
  }
  hip_buffer(const hip_buffer&) = delete;
  hip_buffer& operator=(const hip_buffer&) = delete;
  ~hip_buffer() { reset(); }

  // what it held is freed first; empty again after an error
  hipError_t alloc(size_t count) {
    reset();
    void* p = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&p, sizeof(T) * count, hipHostMallocDefault) : hipMalloc(&p, sizeof(T) * count);
    if (e == hipSuccess) p_ = static_cast<T*>(p);
    return e;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }  // (the host never dereferences it; a copy of the owner does not compile)
  void reset() {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
  }

 private:
  T* p_ = nullptr;
};

template <class T>
using device_buffer = hip_buffer<T, false>;
template <class T>
using pinned_buffer = hip_buffer<T, true>;

// hipStream_t / hipEvent_t, destroyed with their owner; empty until hip_steps::stream / ::event (or create) has made them
template <class H, hipError_t (*Destroy)(H)>
class hip_handle {
 public:
  hip_handle() = default;
  hip_handle(hip_handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  hip_handle& operator=(hip_handle&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, nullptr);
    }
    return *this;
  }
  hip_handle(const hip_handle&) = delete;
  hip_handle& operator=(const hip_handle&) = delete;
  ~hip_handle() { reset(); }
  H get() const { return h_; }
  operator H() const { return h_; }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }

 protected:
  H h_ = nullptr;
};

struct hip_stream : hip_handle<hipStream_t, hipStreamDestroy> {
  hipError_t create() {  // non-blocking, as every stream of the library is
    reset();
    return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking);
  }
};

struct hip_event : hip_handle<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDisableTiming) {
    reset();
    return hipEventCreateWithFlags(&h_, flags);
  }
};

// a grow frees everything it replaces before it allocates anything
template <class... B>
void reset_all(B&... b) {
  (b.reset(), ...);
}

// hip_steps().alloc(a, n).alloc(b, m).then([&] { return hipMemsetAsync(...); }, "hipMemsetAsync"): every step behind the first error is
// skipped; error() is that error and what() names the call that gave it, for "<call> failed: <error>"
class hip_steps {
 public:
  template <class T, bool Pinned>
  hip_steps& alloc(hip_buffer<T, Pinned>& b, size_t count) {
    if (err_ == hipSuccess && (err_ = b.alloc(count)) != hipSuccess) snprintf(what_, sizeof(what_), "%s of %zu bytes", Pinned ? "hipHostMalloc" : "hipMalloc", sizeof(T) * count);
    return *this;
  }
  hip_steps& stream(hip_stream& s) {
    return then([&] { return s.create(); }, "hipStreamCreateWithFlags");
  }
  hip_steps& event(hip_event& e, unsigned flags = hipEventDisableTiming) {
    return then([&] { return e.create(flags); }, "hipEventCreateWithFlags");
  }
  // the first `count` elements of b, zeroed on `s`
  template <class T>
  hip_steps& zero_async(const device_buffer<T>& b, size_t count, hipStream_t s) {
    return then([&] { return hipMemsetAsync(b.get(), 0, sizeof(T) * count, s); }, "hipMemsetAsync");
  }
  // allocate for and copy (synchronously) what a host vector holds
  template <class T>
  hip_steps& upload(device_buffer<T>& b, const std::vector<T>& host) {
    alloc(b, host.size());
    return then([&] { return hipMemcpy(b.get(), host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice); }, "hipMemcpy");
  }
  template <class F>
  hip_steps& then(F&& call, const char* name = "a HIP call") {
    if (err_ == hipSuccess && (err_ = call()) != hipSuccess) snprintf(what_, sizeof(what_), "%s", name);
    return *this;
  }
  bool ok() const { return err_ == hipSuccess; }
  hipError_t error() const { return err_; }
  const char* what() const { return what_; }

 private:
  hipError_t err_ = hipSuccess;
  char what_[64] = "";
};

}  // namespace
}  // namespace ss
