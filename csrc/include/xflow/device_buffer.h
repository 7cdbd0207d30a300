// xflow-amd: DeviceBuffer -- one owned array of backend memory.
//
// Move-only; frees itself by kind, so an owner needs no free list and a
// constructor that throws leaks nothing.  The owner's Backend must outlive
// the buffer (declare it first).  Kernel argument structs keep taking raw
// pointers: a buffer converts to T*.
#pragma once

#include <cstddef>
#include <utility>

#include "xflow/backend.h"

namespace xflow {

enum class Mem {
  kDevice,   // Backend::alloc / free (a growth waits for the stream first)
  kStream,   // alloc_stream / free_stream: stream-ordered, no host wait
  kHost,     // host_alloc / host_free: pinned, zeroed
  kStaging,  // staging_alloc / staging_free: pinned DMA staging
};

template <typename T, Mem K = Mem::kDevice>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(Backend& be, size_t n) { alloc(be, n); }
  DeviceBuffer(DeviceBuffer&& o) noexcept { *this = std::move(o); }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {  // (o frees what this held)
    std::swap(be_, o.be_);
    std::swap(p_, o.p_);
    std::swap(cap_, o.cap_);
    return *this;
  }
  ~DeviceBuffer() { reset(); }

  T* get() const { return p_; }
  T* data() const { return p_; }
  operator T*() const { return p_; }
  size_t capacity() const { return cap_; }  // elements

  // n elements (at least one is allocated); any old array is freed first
  T* alloc(Backend& be, size_t n) {
    reset();
    const size_t bytes = sizeof(T) * (n ? n : 1);
    be_ = &be;
    p_ = static_cast<T*>(K == Mem::kDevice   ? be.alloc(bytes)
                         : K == Mem::kStream ? be.alloc_stream(bytes)
                         : K == Mem::kHost   ? be.host_alloc(bytes)
                                             : be.staging_alloc(bytes));
    cap_ = n;
    return p_;
  }
  // ... then zeroed on the backend's stream
  T* alloc_zero(Backend& be, size_t n) {
    be.memset(alloc(be, n), 0, sizeof(T) * n);
    return p_;
  }
  // allocate-once buffers: n elements on first use
  T* ensure(Backend& be, size_t n) { return p_ ? p_ : alloc(be, n); }
  // Grow-only: below `need` elements, re-allocate to new_cap (the caller's
  // slack rule); the contents are not kept.  Returns whether it grew.  A
  // plain device array may still be read by queued work, so the stream is
  // drained before it is freed; a stream-ordered one is freed behind that work.
  bool reserve(Backend& be, size_t need, size_t new_cap) {
    if (need <= cap_) return false;
    if (K == Mem::kDevice) be.synchronize();
    alloc(be, new_cap);
    return true;
  }
  void reset() {
    if (p_) {
      if (K == Mem::kDevice) be_->free(p_);
      else if (K == Mem::kStream) be_->free_stream(p_);
      else if (K == Mem::kHost) be_->host_free(p_);
      else be_->staging_free(p_);
    }
    p_ = nullptr;
    cap_ = 0;
  }

 private:
  Backend* be_ = nullptr;
  T* p_ = nullptr;
  size_t cap_ = 0;
};

template <typename T>
using StreamBuffer = DeviceBuffer<T, Mem::kStream>;
template <typename T>
using HostBuffer = DeviceBuffer<T, Mem::kHost>;

}  // namespace xflow
