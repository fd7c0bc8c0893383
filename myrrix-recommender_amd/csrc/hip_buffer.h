// hip_buffer.h -- the owners of what the library takes from the HIP runtime (host code only): every block of device or
// pinned host memory (HipBuffer), every event (Event, EventPair) and every stream (Stream) it creates.  An owner releases
// what it holds when it is reset, assigned to or destroyed -- a buffer also when it is reallocated -- so a holder's teardown
// lists nothing, and a half-built holder leaks nothing.  What the library only borrows stays raw: caller-bound factors, an
// installed ingest's matrices, views into an owned block, the caller's stream (mals_set_stream), every hipStream_t /
// hipEvent_t parameter.  Fallible calls return the hipError_t of the call that failed.
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

// ---- events and streams ------------------------------------------------------------------------------------------
// The runtime calls of the two owners below, as a policy (a host test puts a recording fake in their place).
struct HipEventApi {
  static hipError_t create(hipEvent_t* e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
  static void destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
};
struct HipStreamApi {
  static hipError_t create(hipStream_t* s, unsigned flags) { return hipStreamCreateWithFlags(s, flags); }
  static void synchronize(hipStream_t s) { (void)hipStreamSynchronize(s); }
  static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
};

// An event: empty until ensure(), destroyed on reset, assignment and destruction.  Converts to the raw handle, so it is
// passed to HIP calls as it stands.
template <typename Api>
class BasicEvent {
 public:
  BasicEvent() = default;
  BasicEvent(const BasicEvent&) = delete;
  BasicEvent& operator=(const BasicEvent&) = delete;
  BasicEvent(BasicEvent&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  BasicEvent& operator=(BasicEvent&& o) noexcept {
    if (this != &o) {
      reset();
      e_ = o.e_;
      o.e_ = nullptr;
    }
    return *this;
  }
  ~BasicEvent() { reset(); }

  hipEvent_t get() const { return e_; }
  operator hipEvent_t() const { return e_; }
  explicit operator bool() const { return e_ != nullptr; }

  void reset() {
    if (e_) Api::destroy(e_);
    e_ = nullptr;
  }

  // creates the event unless there is one (whose flags then stay); a failure leaves the owner empty
  hipError_t ensure(unsigned flags = hipEventDefault) {
    if (e_) return hipSuccess;
    hipEvent_t q = nullptr;
    const hipError_t e = Api::create(&q, flags);
    if (e == hipSuccess) e_ = q;
    return e;
  }

 private:
  hipEvent_t e_ = nullptr;
};

// A stream, the same; it is synchronised before it is destroyed, so nothing it ran is in flight once its owner is gone.
// A holder whose buffers the stream's work uses still waits for it itself before it lets go of the first of them.
template <typename Api>
class BasicStream {
 public:
  BasicStream() = default;
  BasicStream(const BasicStream&) = delete;
  BasicStream& operator=(const BasicStream&) = delete;
  BasicStream(BasicStream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  BasicStream& operator=(BasicStream&& o) noexcept {
    if (this != &o) {
      reset();
      s_ = o.s_;
      o.s_ = nullptr;
    }
    return *this;
  }
  ~BasicStream() { reset(); }

  hipStream_t get() const { return s_; }
  operator hipStream_t() const { return s_; }
  explicit operator bool() const { return s_ != nullptr; }

  void reset() {
    if (s_) {
      Api::synchronize(s_);
      Api::destroy(s_);
    }
    s_ = nullptr;
  }

  hipError_t ensure(unsigned flags = hipStreamNonBlocking) {
    if (s_) return hipSuccess;
    hipStream_t q = nullptr;
    const hipError_t e = Api::create(&q, flags);
    if (e == hipSuccess) s_ = q;
    return e;
  }

 private:
  hipStream_t s_ = nullptr;
};

// the two events around a timed stretch of a stream; after a failure halfway the next ensure() completes the pair
template <typename Api>
struct BasicEventPair {
  BasicEvent<Api> begin, end;
  hipError_t ensure(unsigned flags = hipEventDefault) {
    const hipError_t e = begin.ensure(flags);
    return e != hipSuccess ? e : end.ensure(flags);
  }
};

using Event = BasicEvent<HipEventApi>;
using Stream = BasicStream<HipStreamApi>;
using EventPair = BasicEventPair<HipEventApi>;

}  // namespace mals
