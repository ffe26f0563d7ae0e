// hfcl_own.hpp -- owning handles of the host side's device resources: a typed device buffer, a pinned host buffer, a stream, an event.
// Move-only; the destructor gives back what the handle holds (an empty or moved-from handle holds nothing); the raw pointer / handle is
// read through get() or the implicit conversion, so launch code and parameter blocks take them as they took the raw fields.  Errors are
// hipError_t values for the caller's HIP_TRY: no exceptions, no allocator, no pool, no sharing.  Only this header calls hipFree /
// hipHostFree / hipStreamDestroy / hipEventDestroy.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>

// handles alive in this process, per kind (hfcl_debug_live_handles reads them: a library gives back what it took)
enum { HFCL_LIVE_DEVICE = 0, HFCL_LIVE_PINNED = 1, HFCL_LIVE_STREAM = 2, HFCL_LIVE_EVENT = 3 };
inline std::atomic<int64_t> g_hfcl_live[4];

template <typename H, int KIND>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, nullptr);
    }
    return *this;
  }
  ~Owned() { reset(); }
  H get() const { return h_; }
  operator H() const { return h_; }
  void reset() {
    if (!h_) return;
    if constexpr (KIND == HFCL_LIVE_DEVICE) (void)hipFree((void*)h_);  // (waits for the device)
    else if constexpr (KIND == HFCL_LIVE_PINNED) (void)hipHostFree((void*)h_);
    else if constexpr (KIND == HFCL_LIVE_STREAM) (void)hipStreamDestroy(h_);
    else (void)hipEventDestroy(h_);
    g_hfcl_live[KIND].fetch_sub(1, std::memory_order_relaxed);
    h_ = nullptr;
  }

 protected:
  // takes what a create / allocate call left in `h` (nothing when it failed)
  hipError_t adopt(hipError_t e, H h) {
    h_ = e == hipSuccess ? h : nullptr;
    if (h_) g_hfcl_live[KIND].fetch_add(1, std::memory_order_relaxed);
    return e;
  }
  H h_ = nullptr;
};

// T[capacity()] of device memory (DevBuf<void>: capacity() bytes)
template <typename T>
class DevBuf : public Owned<T*, HFCL_LIVE_DEVICE> {
  using Base = Owned<T*, HFCL_LIVE_DEVICE>;
  static constexpr size_t ELEM = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
  size_t cap_ = 0;

 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : Base(std::move(o)), cap_(std::exchange(o.cap_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    Base::operator=(std::move(o));
    cap_ = std::exchange(o.cap_, 0);
    return *this;
  }
  size_t capacity() const { return cap_; }
  void reset() {
    Base::reset();
    cap_ = 0;
  }
  // Room for n elements: nothing when they fit; otherwise the old buffer is freed FIRST (the two generations never coexist, and hipFree
  // waits for the device: nothing in flight reads the old one), then exactly n are allocated -- the caller chooses the padding.  On
  // failure the buffer is empty with capacity 0, and the next call tries again.
  hipError_t grow(size_t n) {
    if (n <= cap_) return hipSuccess;
    reset();
    void* p = nullptr;
    const hipError_t e = this->adopt(hipMalloc(&p, n * ELEM), static_cast<T*>(p));
    if (e == hipSuccess) cap_ = n;
    return e;
  }
};
template <typename... B>
inline void reset_all(B&... b) { (b.reset(), ...); }

template <typename T>
class PinnedBuf : public Owned<T*, HFCL_LIVE_PINNED> {
 public:
  hipError_t alloc(size_t n) {  // (an empty buffer's first and only allocation)
    void* p = nullptr;
    return this->adopt(hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault), static_cast<T*>(p));
  }
};

class Stream : public Owned<hipStream_t, HFCL_LIVE_STREAM> {
 public:
  hipError_t create() {  // non-blocking, as every stream of the host side
    hipStream_t s = nullptr;
    return adopt(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), s);
  }
  hipError_t create_with_priority(int priority) {
    hipStream_t s = nullptr;
    return adopt(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority), s);
  }
};

class Event : public Owned<hipEvent_t, HFCL_LIVE_EVENT> {
 public:
  hipError_t create(unsigned flags = hipEventDisableTiming) {  // (hipEventDefault: an event that is timed)
    hipEvent_t e = nullptr;
    return adopt(hipEventCreateWithFlags(&e, flags), e);
  }
};
