// Owners of the library's device and pinned-host allocations.  Every handle struct keeps its buffers as DevBuf / HostPinned members, so a handle's
// destructor frees what it owns and a create function that fails half way leaves nothing behind.  A pointer that is borrowed stays a raw pointer.
// The runtime is reached only through the seam below (ins_devmem.hip): this header needs no HIP header and compiles with a plain host compiler.
#pragma once

#include <cstddef>
#include <cstdint>

#include "ins_hip.h"

// The seam.  The int-returning calls give INS_OK or INS_ERR_HIP and record a message (with the size) through ins_set_error; a failed allocation stores
// nullptr.  `stream` is a hipStream_t.  ins_devmem_live: buffers and bytes handed out and not yet freed (device and pinned host together).
int ins_devmem_alloc(void** p, size_t bytes);
void ins_devmem_free(void* p, size_t bytes);
int ins_devmem_zero(void* p, size_t bytes);
int ins_devmem_zero_async(void* p, size_t bytes, void* stream);
int ins_devmem_copy_from_host(void* dst, const void* src, size_t bytes);                 // blocking
int ins_devmem_copy_on_device(void* dst, const void* src, size_t bytes, void* stream);  // stream-ordered
int ins_devmem_host_alloc(void** p, size_t bytes);
void ins_devmem_host_free(void* p, size_t bytes);
void ins_devmem_live(int64_t* buffers, int64_t* bytes);

// One device allocation of count() elements of T.  Move-only; null by default; converts to T* so that launches and pointer arithmetic read as before.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t count() const { return n_; }
  void reset() {
    if (p_) ins_devmem_free(p_, n_ * sizeof(T));
    p_ = nullptr, n_ = 0;
  }

  // Each form frees what the buffer held, allocates `count` elements and fills them as named; on failure the buffer is null.
  int alloc(size_t count) {
    reset();
    void* p = nullptr;
    int rc = ins_devmem_alloc(&p, count * sizeof(T));
    if (rc == INS_OK) p_ = static_cast<T*>(p), n_ = count;
    return rc;
  }
  int alloc_zero(size_t count) { return filled(alloc(count), [&] { return ins_devmem_zero(p_, n_ * sizeof(T)); }); }
  int alloc_zero_async(size_t count, void* stream) { return filled(alloc(count), [&] { return ins_devmem_zero_async(p_, n_ * sizeof(T), stream); }); }
  int alloc_copy_host(size_t count, const T* src) { return filled(alloc(count), [&] { return ins_devmem_copy_from_host(p_, src, n_ * sizeof(T)); }); }
  int alloc_copy_device(size_t count, const T* src, void* stream) {
    return filled(alloc(count), [&] { return ins_devmem_copy_on_device(p_, src, n_ * sizeof(T), stream); });
  }
  // At least `count` elements: nothing happens when the buffer is that large already (its address stays), else it is freed and allocated anew, unfilled.
  int ensure(size_t count) { return p_ && n_ >= count ? INS_OK : alloc(count); }

 private:
  template <typename F>
  int filled(int rc, F fill) {
    if (rc == INS_OK && n_ && (rc = fill()) != INS_OK) reset();
    return rc;
  }
  T* p_ = nullptr;
  size_t n_ = 0;
};

// The same for pinned host memory (the mirrors of device scalars the blocking reductions and the CG iteration read).
template <typename T>
class HostPinned {
 public:
  HostPinned() = default;
  HostPinned(const HostPinned&) = delete;
  HostPinned& operator=(const HostPinned&) = delete;
  HostPinned(HostPinned&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  HostPinned& operator=(HostPinned&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  ~HostPinned() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t count() const { return n_; }
  void reset() {
    if (p_) ins_devmem_host_free(p_, n_ * sizeof(T));
    p_ = nullptr, n_ = 0;
  }
  int alloc(size_t count) {
    reset();
    void* p = nullptr;
    int rc = ins_devmem_host_alloc(&p, count * sizeof(T));
    if (rc == INS_OK) p_ = static_cast<T*>(p), n_ = count;
    return rc;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};
