// hip_buffer.h -- the owner of every block of device or pinned host memory the library allocates (host code only).
// A buffer knows its block and its capacity in elements; it releases the block when it is reset, reallocated, assigned
// to or destroyed.  Memory the library only borrows (caller-bound factors, an installed ingest's matrices) stays a raw
// pointer, and so do views into an owned block.  Fallible calls return the hipError_t of the call that failed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <utility>

namespace mals {

struct DeviceMemory {
  static hipError_t acquire(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
};
struct PinnedMemory {
  static hipError_t acquire(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void* p) { (void)hipHostFree(p); }
};

template <typename T, typename Memory>
class HipBuffer {
 public:
  HipBuffer() = default;
  HipBuffer(const HipBuffer&) = delete;
  HipBuffer& operator=(const HipBuffer&) = delete;
  HipBuffer(HipBuffer&& o) noexcept : p_(o.p_), cap_(o.cap_) {
    o.p_ = nullptr;
    o.cap_ = 0;
  }
  HipBuffer& operator=(HipBuffer&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      cap_ = o.cap_;
      o.p_ = nullptr;
      o.cap_ = 0;
    }
    return *this;
  }
  ~HipBuffer() { reset(); }

  T* get() const { return p_; }
  size_t capacity() const { return cap_; }  // elements
  explicit operator bool() const { return p_ != nullptr; }

  void reset() {
    if (p_) Memory::release(p_);
    p_ = nullptr;
    cap_ = 0;
  }

  // exactly n elements; the old block is released first (capacity 0 until the new one exists).  A failure is returned,
  // not left pending as well: the next hipGetLastError (a kernel launch check) must not report it a second time.
  hipError_t alloc(size_t n) {
    reset();
    void* q = nullptr;
    const hipError_t e = Memory::acquire(&q, sizeof(T) * n);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return e;
    }
    p_ = static_cast<T*>(q);
    cap_ = n;
    return hipSuccess;
  }

  // grow-only: when n exceeds the capacity, wait for `stream` (work in flight may still use the old block), release,
  // allocate exactly n
  hipError_t reserve(size_t n, hipStream_t stream) {
    if (n <= cap_) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    return alloc(n);
  }

  // a new block of n elements that starts with the first `used` elements of the old one (copied on `stream`, which is
  // then synchronised); the old block is released once the new one holds them.  Device memory only.
  hipError_t grow_keep(size_t n, size_t used, hipStream_t stream) {
    static_assert(std::is_same<Memory, DeviceMemory>::value, "grow_keep copies device to device");
    HipBuffer q;
    hipError_t e = q.alloc(n);
    if (e == hipSuccess && used) e = hipMemcpyAsync(q.p_, p_, sizeof(T) * used, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess && used) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    *this = std::move(q);
    return hipSuccess;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

template <typename T>
using DeviceBuffer = HipBuffer<T, DeviceMemory>;
template <typename T>
using PinnedBuffer = HipBuffer<T, PinnedMemory>;

// the two events around a timed stretch of a stream, destroyed with their holder on whichever path it is left
struct EventPair {
  hipEvent_t begin = nullptr, end = nullptr;
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  ~EventPair() {
    if (begin) (void)hipEventDestroy(begin);
    if (end) (void)hipEventDestroy(end);
  }
  hipError_t create() {
    const hipError_t e = hipEventCreate(&begin);
    return e != hipSuccess ? e : hipEventCreate(&end);
  }
};

}  // namespace mals
