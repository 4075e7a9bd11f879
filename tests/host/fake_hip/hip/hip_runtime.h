// A stand-in for <hip/hip_runtime.h>, just enough of it for csrc/device_buffers.h and csrc/ctx_buffers.h to compile with g++ and run
// without a GPU (tests/host/ctx_buffers_check.cpp). Device and pinned memory are small heap blocks (the sanitizer sees every leak and
// double free; the requested size is recorded, not allocated: a context asks for gigabytes), streams and events are heap objects,
// memset and memcpy only check that what they are given is live, and the n-th call can be made to fail.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
struct float2 {
  float x, y;
};
struct fake_stream {
  int unused;
};
struct fake_event {
  int unused;
};
typedef fake_stream* hipStream_t;
typedef fake_event* hipEvent_t;
constexpr unsigned hipStreamNonBlocking = 1, hipEventDefault = 0, hipEventDisableTiming = 2, hipHostMallocDefault = 0;

namespace fake_hip {
struct State {
  std::set<const void*> live;  // blocks, streams and events that exist
  std::vector<size_t> sizes;   // bytes asked of hipMalloc, in call order
  long calls = 0, fail_at = -1;
  std::string failed;  // the call that was made to fail
  int bad = 0;         // a pointer used or freed that is not live
};
inline State& state() {
  static State s;
  return s;
}
inline bool fails(const char* name) {
  if (state().calls++ != state().fail_at) return false;
  state().failed = name;
  return true;
}
inline hipError_t use(const void* p) {
  if (state().live.count(p)) return hipSuccess;
  ++state().bad;
  return hipErrorInvalidValue;
}
template <class T>
hipError_t make(T** out, const char* name, hipError_t err) {
  if (fails(name)) return err;
  *out = static_cast<T*>(malloc(sizeof(T) < 16 ? 16 : sizeof(T)));
  state().live.insert(*out);
  return hipSuccess;
}
template <class T>
hipError_t drop(T* p) {
  if (!state().live.erase(p)) {
    ++state().bad;
    return hipErrorInvalidValue;
  }
  free(p);
  return hipSuccess;
}
}  // namespace fake_hip

inline hipError_t hipMalloc(void** p, size_t bytes) {
  const hipError_t e = fake_hip::make(reinterpret_cast<char**>(p), "hipMalloc", hipErrorOutOfMemory);
  if (e == hipSuccess) fake_hip::state().sizes.push_back(bytes);
  return e;
}
inline hipError_t hipHostMalloc(void** p, size_t, unsigned) { return fake_hip::make(reinterpret_cast<char**>(p), "hipHostMalloc", hipErrorOutOfMemory); }
inline hipError_t hipFree(void* p) { return fake_hip::drop(static_cast<char*>(p)); }
inline hipError_t hipHostFree(void* p) { return fake_hip::drop(static_cast<char*>(p)); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return fake_hip::make(s, "hipStreamCreateWithFlags", hipErrorOutOfMemory); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake_hip::drop(s); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return fake_hip::make(e, "hipEventCreateWithFlags", hipErrorOutOfMemory); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake_hip::drop(e); }
inline hipError_t hipMemset(void* p, int, size_t) { return fake_hip::fails("hipMemset") ? hipErrorInvalidValue : fake_hip::use(p); }
inline hipError_t hipMemsetAsync(void* p, int, size_t, hipStream_t s) {
  if (fake_hip::fails("hipMemsetAsync")) return hipErrorInvalidValue;
  const hipError_t e = fake_hip::use(p);
  return e != hipSuccess ? e : fake_hip::use(s);
}
inline hipError_t hipMemcpy(void* dst, const void*, size_t, hipMemcpyKind) { return fake_hip::fails("hipMemcpy") ? hipErrorInvalidValue : fake_hip::use(dst); }
