// er_mem.h -- who frees device and page-locked host memory, decided once: a scope of allocations (everything a call or a handle allocated, freed
// together) and a grow-only buffer (one array with a capacity).  Host code only; needs nothing beyond er_common.h.  A request for zero elements
// allocates a minimal block, so no caller clamps a size; a failed allocation leaves a null pointer whatever the runtime did to the out-pointer
// (a failing hipMalloc leaves it untouched) and reports through er::fail as "<who>: hipMalloc(<bytes> bytes) failed: <HIP error>".
#pragma once

#include "er_common.h"

#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

namespace er {

enum class Mem { Device, Pinned };

constexpr size_t kMemMinBytes = 16;   // what a request for zero elements gets: the runtime is never asked for 0 bytes

// One raw allocation of max(bytes, kMemMinBytes) bytes: *out is the block, or nullptr after er::fail.
template <Mem K>
__attribute__((visibility("hidden"))) inline int mem_alloc(void** out, size_t bytes, const char* who) {
  void* p = nullptr;
  const size_t n = std::max(bytes, kMemMinBytes);
  hipError_t e = K == Mem::Device ? hipMalloc(&p, n) : hipHostMalloc(&p, n, hipHostMallocDefault);
  *out = e == hipSuccess ? p : nullptr;
  if (e == hipSuccess) return 0;
  return fail("%s: %s(%zu bytes) failed: %s", who, K == Mem::Device ? "hipMalloc" : "hipHostMalloc", bytes, hipGetErrorString(e));
}

template <Mem K>
__attribute__((visibility("hidden"))) inline void mem_free(void* p) {
  if (p) (void)(K == Mem::Device ? hipFree(p) : hipHostFree(p));
}

template <typename T>
constexpr size_t mem_elem_size() {
  if constexpr (std::is_void<T>::value) return 1;   // a void* array is counted in bytes
  else return sizeof(T);
}

// Device allocations that live and die together: those of one call (freed however the call leaves), or the fixed ones of a handle.
class __attribute__((visibility("hidden"))) DevScope {
 public:
  DevScope() = default;
  DevScope(const DevScope&) = delete;
  DevScope& operator=(const DevScope&) = delete;
  DevScope(DevScope&& o) noexcept : held_(std::move(o.held_)) { o.held_.clear(); }
  DevScope& operator=(DevScope&& o) noexcept {
    if (this != &o) {
      free_all();
      held_ = std::move(o.held_);
      o.held_.clear();
    }
    return *this;
  }
  ~DevScope() { free_all(); }

  // *out = `count` elements of device memory that this scope frees, or nullptr (returns 1, er::fail has the text).
  template <typename T>
  int alloc(T** out, size_t count, const char* who) {
    void* p = nullptr;
    int rc = mem_alloc<Mem::Device>(&p, count * mem_elem_size<T>(), who);
    *out = static_cast<T*>(p);
    if (!rc) held_.push_back(p);
    return rc;
  }
  // Hands one allocation to the caller, who frees it from now on; a pointer this scope does not hold is left alone.
  template <typename T>
  T* release(T* p) {
    auto it = std::find(held_.begin(), held_.end(), static_cast<const void*>(p));
    if (it != held_.end()) held_.erase(it);
    return p;
  }
  void free_all() {
    for (void* p : held_) mem_free<Mem::Device>(p);
    held_.clear();
  }

 private:
  std::vector<void*> held_;
};

// One array of T that only grows: reserve(n) keeps the block when it is large enough and otherwise replaces it (contents are not kept).
template <typename T, Mem K = Mem::Device>
class __attribute__((visibility("hidden"))) Buffer {
 public:
  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  ~Buffer() { reset(); }

  // Room for n elements; on failure (returns 1) the buffer is empty.
  int reserve(size_t n, const char* who) {
    if (p_ && n <= cap_) return 0;
    reset();
    void* p = nullptr;
    if (mem_alloc<K>(&p, n * mem_elem_size<T>(), who)) return 1;
    p_ = static_cast<T*>(p);
    cap_ = n;
    return 0;
  }
  void reset() {
    mem_free<K>(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t capacity() const { return cap_; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

template <typename T>
using PinnedBuffer = Buffer<T, Mem::Pinned>;

}  // namespace er
