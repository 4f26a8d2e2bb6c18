// egm_buf.h — the two owning buffers of the host side: device memory and
// pinned host memory, each grown on demand and freed with its owner.
// Internal to the library (hidden visibility: nothing here is exported).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

#pragma GCC visibility push(hidden)
namespace egm {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
  }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    release();
    size_t b = bytes < 256 ? 256 : bytes;
    hipError_t e = hipMalloc(&p, b);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = b;
    return hipSuccess;
  }
  template <class T>
  T* as() const { return (T*)p; }
};

// Pinned host memory (page-locked: DMA at full PCIe rate, asynchronous copies).
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { release(); }
  void release() {
    if (p) hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  // `alloc`: the size to pin when `bytes` does not fit (0: a quarter of headroom)
  hipError_t ensure(size_t bytes, size_t alloc = 0) {
    if (bytes <= cap && p) return hipSuccess;
    release();
    const size_t b = alloc ? alloc : bytes + bytes / 4 + 4096;   // grow with headroom: pinning is slow
    hipError_t e = hipHostMalloc(&p, b, hipHostMallocDefault);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = b;
    return hipSuccess;
  }
};

}  // namespace egm
#pragma GCC visibility pop
