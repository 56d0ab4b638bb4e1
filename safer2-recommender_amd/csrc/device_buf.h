// device_buf.h -- the owners of the HIP resources a context holds (host
// only): one device allocation (DevBuf), one pinned staging buffer
// (PinnedBuf), a stream and an event.  Each is move-only and gives its
// resource back in its destructor, so a context member cannot be forgotten
// in a teardown list.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace frecsys_hip {

// Bytes every DevBuf of the process holds now (frecsys_counter
// "live_device_bytes"): process-wide, so it can still be read once a
// context is gone.
inline std::atomic<int64_t>& live_device_bytes() {
  static std::atomic<int64_t> bytes{0};
  return bytes;
}

// One hipMalloc allocation of `cap()` elements.  reserve() keeps the
// allocation whenever it is large enough -- the same pointer, no hipFree
// (which synchronises the device) -- and otherwise frees it and allocates
// exactly the request.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  ~DevBuf() { (void)release(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }  // elements asked for; 0 when empty
  size_t bytes() const { return p_ ? sizeof(T) * std::max<size_t>(cap_, 1) : 0; }

  // Frees the allocation, if any.  On an error the buffer keeps it.
  hipError_t release() {
    if (p_) {
      const hipError_t e = hipFree(p_);
      if (e != hipSuccess) return e;
      live_device_bytes() -= (int64_t)bytes();
    }
    p_ = nullptr;
    cap_ = 0;
    return hipSuccess;
  }

  // Room for `count` elements (at least one is allocated).  On an error the
  // buffer is empty, unless the hipFree failed: then it keeps what it had.
  hipError_t reserve(size_t count) {
    if (cap_ >= count && p_) return hipSuccess;
    hipError_t e = release();
    if (e != hipSuccess) return e;
    e = hipMalloc((void**)&p_, sizeof(T) * std::max<size_t>(count, 1));
    if (e != hipSuccess) {
      p_ = nullptr;
      return e;
    }
    cap_ = count;
    live_device_bytes() += (int64_t)bytes();
    return hipSuccess;
  }

  // reserve() that reports an out-of-memory hipMalloc instead of failing:
  // *oom is set, the buffer left empty and HIP's sticky last error cleared
  // (the next launch check would otherwise see it).
  hipError_t try_reserve(size_t count, bool* oom) {
    *oom = false;
    const hipError_t e = reserve(count);
    if (e == hipSuccess || p_) return e;  // fine, or the hipFree failed
    (void)hipGetLastError();
    if (e != hipErrorOutOfMemory) return e;
    *oom = true;
    return hipSuccess;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// One hipHostMalloc staging buffer; grows only.
template <typename T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  PinnedBuf(PinnedBuf&& o) noexcept
      : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  ~PinnedBuf() { (void)release(); }

  T* get() const { return p_; }

  hipError_t release() {
    if (p_) {
      const hipError_t e = hipHostFree(p_);
      if (e != hipSuccess) return e;
    }
    p_ = nullptr;
    cap_ = 0;
    return hipSuccess;
  }

  hipError_t reserve(size_t count) {
    if (cap_ >= count) return hipSuccess;
    hipError_t e = release();
    if (e != hipSuccess) return e;
    e = hipHostMalloc((void**)&p_, sizeof(T) * std::max<size_t>(count, 1), hipHostMallocDefault);
    if (e != hipSuccess) {
      p_ = nullptr;
      return e;
    }
    cap_ = count;
    return hipSuccess;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// A stream / an event the holder created (assigned through `h`); destroyed
// with it.  The holder synchronises a stream before it lets go of it.
struct Stream {
  hipStream_t h = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (h) (void)hipStreamDestroy(h);
  }
  operator hipStream_t() const { return h; }
};

struct Event {
  hipEvent_t h = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  ~Event() {
    if (h) (void)hipEventDestroy(h);
  }
  operator hipEvent_t() const { return h; }
};

}  // namespace frecsys_hip
