// ns_api_int.h — what the translation units behind the C ABI share: ns_api.cpp (error string, device, tuning, thin device-pointer
// wrappers), ns_weights.cpp (blob -> device weight, cache), ns_dispatch.cpp (which kernel serves a forward) and ns_host_entry.cpp (the
// reference's host-pointer surface).  Not installed; everything one of those files uses alone stays local to it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ns_bestla.h"
#include "ns_common.h"

namespace ns {

// ---- ns_api.cpp ----
bool hip_ok(hipError_t e, const char* what);  // false + error string "<what>: <HIP's text>"
bool have_device();                           // false + error string without a HIP device; every compute entry passes here first
// A launcher that may decline a shape.  true: the call is decided, *rc is its return code (error string "<what>: ..." on failure);
// false: hipErrorNotSupported — outside that launcher's envelope, the caller's next path serves the call.
bool launched(hipError_t e, const char* what, int* rc);

template <typename T>
struct DevBuf {
  T* p = nullptr;
  ~DevBuf() {
    if (p) hipFree(p);
  }
  bool alloc(size_t count) { return hip_ok(hipMalloc((void**)&p, count * sizeof(T) + 16), "hipMalloc(temp)"); }
};

// ---- ns_weights.cpp ----
ns_weight* cached_weight(const void* blob);  // host blob pointer -> device weight (loaded on first sight); nullptr + error string
// Pinning against the NS_CACHE_MAX_BYTES eviction: every host entry that looks weights up opens a CachePin for its duration
struct CachePin {
  CachePin();
  ~CachePin();
  CachePin(const CachePin&) = delete;
  CachePin& operator=(const CachePin&) = delete;
};
void set_planes_load(int on);  // ns_hip_set_tuning("planes_load")

// ---- ns_dispatch.cpp ----
// the quantization format of two weights agrees: kind, group size, scale type, asymmetry, code type (shapes are the caller's business)
bool same_quant(const ns_weight* a, const ns_weight* b);
int forward_impl(const float* dA, const ns_weight* w, float* dC, int m, int lda, int ldc, int epilogue, const float* dD, int ldd,
                 hipStream_t st, const void* dA16 = nullptr, void* dC16 = nullptr, bool reuse_aq = false,
                 const ns_norm_link* link = nullptr);

}  // namespace ns
