// capi_common.h -- what the C ABI's translation units share (t2_capi.cpp: the T2 blocks and the chain;
// stream_capi.cpp: the stream handles beside the chain): the HIP status mapping, device buffers, a handle's device
// and stream.  Internal: nothing here is part of include/dvbt2ll_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "../../include/dvbt2ll_hip.h"

namespace t2 {

// the last HIP error of this thread, which dvbt2ll_strerror(DVBT2LL_EDEVICE) names: one object for the library
inline hipError_t &last_hip_error() {
  static thread_local hipError_t e = hipSuccess;
  return e;
}

#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t e_ = (expr);                             \
    if (e_ != hipSuccess) {                             \
      last_hip_error() = e_;                            \
      return e_ == hipErrorOutOfMemory ? DVBT2LL_ENOMEM : DVBT2LL_EDEVICE; \
    }                                                   \
  } while (0)

// device buffer with grow-on-demand
struct DevBuf {
  void *p = nullptr;
  size_t n = 0;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  int ensure(size_t bytes) {
    if (bytes <= n) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (hipMalloc(&p, bytes) != hipSuccess) return DVBT2LL_ENOMEM;
    n = bytes;
    return 0;
  }
  template <class T> T *as() const { return (T *)p; }
};

template <class T>
int upload(DevBuf &b, const std::vector<T> &v) {
  if (v.empty()) return 0;
  if (b.ensure(v.size() * sizeof(T))) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
inline int upload_raw(DevBuf &b, const void *src, size_t bytes) {
  if (b.ensure(bytes)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

struct DeviceCtx {
  int device = 0;
  hipStream_t stream = nullptr;
  int init(int dev) {
    device = dev;
    HIP_TRY(hipSetDevice(dev));
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return 0;
  }
  ~DeviceCtx() {
    if (stream) { (void)hipSetDevice(device); (void)hipStreamDestroy(stream); }
  }
};

}  // namespace t2
