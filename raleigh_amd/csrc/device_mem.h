// Device memory the library owns on behalf of a handle or a build: one allocation point, one owning type.
// (Free of HIP declarations: tools/device_mem_main.cpp runs DevBuf on the host over malloc / free.)
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rlh {

// Defined in context.hip (the stand-alone test defines its own).
// device_alloc: `bytes` of device memory; sets the error text and returns non-zero on failure (*p is then null).
// device_release: no-op for null and once the context is gone (device_context_live() false: interpreter teardown after
// rlh_finalize).  The two keep the counters that rlh_device_live reports.
int device_alloc(void **p, size_t bytes);
void device_release(void *p);
bool device_context_live();
int device_copy_in(void *dst, const void *src, size_t bytes);      // host to device, blocking
int device_stream_sync();                                          // waits for the library's stream

template <typename T> struct DevElem { static constexpr size_t size = sizeof(T); };
template <> struct DevElem<void> { static constexpr size_t size = 1; };

// Owner of one device allocation.  Converts to T * so that launch sites read like a plain pointer.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; bytes_ = o.bytes_;
      o.p_ = nullptr; o.bytes_ = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  // `count` elements (bytes for DevBuf<void>), uninitialised; what the buffer held is released first
  int alloc(size_t count) { return take(count * DevElem<T>::size); }
  // `bytes` of `src` in a new allocation of max(bytes, at_least) bytes
  int upload(const void *src, size_t bytes, size_t at_least = 0) {
    if (int rc = take(bytes > at_least ? bytes : at_least)) return rc;
    return bytes ? device_copy_in(p_, src, bytes) : 0;
  }
  // grow-only workspace: at least `bytes`, contents not kept; the stream is drained before the old block goes
  int reserve(size_t bytes) {
    if (bytes <= bytes_) return 0;
    if (int rc = device_stream_sync()) return rc;
    return take(bytes);
  }
  void reset() {
    device_release(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  T *get() const { return p_; }
  size_t bytes() const { return bytes_; }
  operator T *() const { return p_; }
  template <typename U> explicit operator U *() const { return (U *)p_; }      // (const U *)buf, as of a plain pointer

 private:
  int take(size_t bytes) {
    reset();
    void *p = nullptr;
    if (int rc = device_alloc(&p, bytes)) return rc;
    p_ = (T *)p;
    bytes_ = bytes;
    return 0;
  }
  T *p_ = nullptr;
  size_t bytes_ = 0;
};

}  // namespace rlh
