// device_mem_check -- csrc/er_mem.h on its own: the scope of device allocations and the grow-only buffer (device and page-locked host memory).
// Without a HIP device the failure path is checked (what a failed allocation leaves behind), with one the success path at the smallest sizes.
// Built from this file and csrc/er_common.cpp alone; prints one line per check and exits non-zero at the first that fails.
#include "er_mem.h"

#include "er_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

namespace {

void check(bool ok, const char* what) {
  printf("%s  %s\n", ok ? "ok  " : "FAIL", what);
  fflush(stdout);
  if (!ok) exit(1);
}

// 1: page-locked host memory, 2: device memory, 0: nothing HIP knows (the test er_icp.hip's buffer_kind makes)
int kind(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return at.type == hipMemoryTypeHost ? 1 : at.type == hipMemoryTypeDevice ? 2 : 0;
}

bool says(const char* who) { return strstr(er_last_error(), who) != nullptr; }

template <er::Mem K>
void buffer_fails(const char* who) {
  er::Buffer<int, K> b;
  check(b.reserve(3, who) == 1 && b.get() == nullptr && b.capacity() == 0, "a failed reserve returns 1 and leaves the buffer empty");
  check(says(who) && strstr(er_last_error(), K == er::Mem::Device ? "hipMalloc(12 bytes)" : "hipHostMalloc(12 bytes)"),
        "its error text names the caller, the call and the size");
  check(b.reserve(0, who) == 1 && b.get() == nullptr && b.capacity() == 0, "so does a failed reserve(0)");
  b.reset();
  er::Buffer<int, K> c(std::move(b));
  b = std::move(c);
  check(b.get() == nullptr && c.get() == nullptr && b.capacity() == 0, "reset and moves of an empty buffer are harmless");
}

void without_device() {
  {
    er::DevScope s;
    int* p = reinterpret_cast<int*>(0x10);                    // (a failing hipMalloc leaves its out-pointer as it was)
    check(s.alloc(&p, 5, "scope_who") == 1, "a failed alloc returns 1");
    check(p == nullptr, "and nulls the out-pointer, whatever it held");
    check(says("scope_who") && strstr(er_last_error(), "hipMalloc(20 bytes)"), "its error text names the caller, the call and the size");
    void* v = reinterpret_cast<void*>(0x20);
    check(s.alloc(&v, 0, "scope_who") == 1 && v == nullptr, "so does a failed alloc of zero bytes");
    int local = 0;
    check(s.release(&local) == &local, "release of a pointer the scope does not hold hands it back");
    s.free_all();
    s.free_all();
    er::DevScope t(std::move(s));
    s = std::move(t);
  }
  check(true, "free_all, moves and the destructor of an empty scope are harmless");
  buffer_fails<er::Mem::Device>("device_who");
  buffer_fails<er::Mem::Pinned>("pinned_who");
}

template <er::Mem K>
void buffer_works(const char* who, int want) {
  void* seen[3] = {nullptr, nullptr, nullptr};
  {
    er::Buffer<int, K> b;
    check(b.reserve(0, who) == 0 && b.get() != nullptr && b.capacity() == 0, "reserve(0) gives a block");
    check(kind(b.get()) == want, "of the right kind of memory");
    int* p0 = b.get();
    check(b.reserve(0, who) == 0 && b.get() == p0, "reserve(0) again keeps it");
    check(b.reserve(5, who) == 0 && b.get() != nullptr && b.capacity() == 5, "a larger n gives capacity n");
    check(b.get() == p0 || kind(p0) == 0, "and frees the block before it (the runtime may hand the same address out again)");
    int* p5 = b.get();
    check(b.reserve(5, who) == 0 && b.reserve(2, who) == 0 && b.get() == p5 && b.capacity() == 5, "n <= capacity keeps pointer and capacity");
    int* q = b;
    check(q == p5 && b + 1 == p5 + 1, "the buffer converts to its pointer");
    er::Buffer<int, K> c(std::move(b));
    check(b.get() == nullptr && b.capacity() == 0 && c.get() == p5 && c.capacity() == 5, "a move takes the block");
    seen[0] = p5;
    er::Buffer<int, K> d;
    check(d.reserve(1, who) == 0, "a second buffer");
    seen[1] = d.get();
    d = std::move(c);
    check(kind(seen[1]) == 0 && d.get() == p5 && kind(p5) == want, "move assignment frees what the target held");
    er::Buffer<int, K> e;
    check(e.reserve(7, who) == 0, "a third buffer");
    seen[2] = e.get();
    e.reset();
    check(e.get() == nullptr && e.capacity() == 0 && kind(seen[2]) == 0, "reset frees and empties");
  }
  check(kind(seen[0]) == 0, "the destructor frees the block");
}

void with_device() {
  check(hipSetDevice(0) == hipSuccess, "hipSetDevice(0)");
  int *a = nullptr, *kept = nullptr;
  double* b = nullptr;
  void* z = nullptr;
  {
    er::DevScope s;
    check(s.alloc(&a, 3, "scope") == 0 && s.alloc(&b, 1, "scope") == 0 && s.alloc(&z, 0, "scope") == 0 && s.alloc(&kept, 4, "scope") == 0,
          "four allocations, one of zero elements");
    check(kind(a) == 2 && kind(b) == 2 && kind(z) == 2 && kind(kept) == 2, "all four are device memory");
    check(s.release(kept) == kept, "release hands one out");
    er::DevScope t(std::move(s));
    s = std::move(t);
    check(kind(a) == 2 && kind(b) == 2, "moves of the scope free nothing");
    int* again = nullptr;
    check(s.alloc(&again, 2, "scope") == 0, "a fifth allocation");
    s.free_all();
    check(kind(a) == 0 && kind(again) == 0, "free_all frees what the scope holds");
    check(s.alloc(&a, 3, "scope") == 0 && kind(a) == 2, "and the scope can be used again");
  }
  check(kind(a) == 0 && kind(b) == 0 && kind(z) == 0, "after the scope is gone none of its pointers is an allocation");
  check(kind(kept) == 2, "the released one still is");
  check(hipMemset(kept, 0, 4 * sizeof(int)) == hipSuccess && hipDeviceSynchronize() == hipSuccess, "and can be written to");
  check(er_device_free(kept) == 0 && kind(kept) == 0, "until the program frees it");
  buffer_works<er::Mem::Device>("device", 2);
  buffer_works<er::Mem::Pinned>("pinned", 1);
}

}  // namespace

int main() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    printf("no device: checking the failure path\n");
    without_device();
  } else {
    printf("%d device(s): checking the success path\n", n);
    with_device();
  }
  printf("OK\n");
  return 0;
}
