// ns_scratch.cpp — grow-only device scratch per (stream, slot) for every launcher of libns_hip.so.  The slots and their owners: enum ScratchSlot, ns_common.h.
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <vector>

#include "ns_common.h"

namespace ns {

// Per-(stream, slot) device scratch, grow-only.  Work on one stream is ordered, so one buffer per stream and purpose is
// enough; two streams never share one.  A buffer that was handed out while its stream was CAPTURING is baked into the
// graph being built: such buffers are never freed or moved again (a larger request gets a new buffer, the old one is
// retired until gemm_scratch_release()).  Allocating during a capture needs the thread's capture mode relaxed for the
// duration of the hipMalloc (what PyTorch's caching allocator does as well), otherwise the capture is invalidated.
static std::mutex g_scratch_mutex;
struct ScratchBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool in_graph = false;
};
static std::map<std::pair<hipStream_t, int>, ScratchBuf> g_scratch;
static std::vector<void*> g_scratch_retired;
static void* stream_scratch_impl(hipStream_t st, size_t bytes, int slot, bool* fresh) {
  std::lock_guard<std::mutex> lock(g_scratch_mutex);
  ScratchBuf& e = g_scratch[{st, slot}];
  if (fresh) *fresh = false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) return nullptr;
  const bool capturing = cs != hipStreamCaptureStatusNone;
  if (e.bytes >= bytes) {
    e.in_graph |= capturing;
    return e.p;
  }
  if (e.p) {
    if (e.in_graph || capturing) {
      g_scratch_retired.push_back(e.p);  // a captured graph may point at it / no synchronous free inside a capture
    } else {
      hipStreamSynchronize(st);
      hipStreamCaptureMode fmode = hipStreamCaptureModeRelaxed;
      hipThreadExchangeStreamCaptureMode(&fmode);
      hipFree(e.p);
      hipThreadExchangeStreamCaptureMode(&fmode);
    }
    e = ScratchBuf{};
  }
  void* p = nullptr;
  // relaxed for the duration of the allocation: in the default (global) mode a hipMalloc invalidates ANY capture in
  // progress in the process, this stream's or another thread's
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  hipThreadExchangeStreamCaptureMode(&mode);
  const hipError_t err = hipMalloc(&p, bytes);
  hipThreadExchangeStreamCaptureMode(&mode);
  if (err != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  e.p = p;
  e.bytes = bytes;
  e.in_graph = capturing;
  if (fresh) *fresh = true;
  return p;
}
void* stream_scratch(hipStream_t st, size_t bytes, int slot) { return stream_scratch_impl(st, bytes, slot, nullptr); }
// the same, zero-filled when (re)allocated — counters that every user leaves at zero again (ns_gemvs.hip: split-K tickets).
void* stream_scratch_zeroed(hipStream_t st, size_t bytes, int slot) {
  bool fresh = false;
  void* p = stream_scratch_impl(st, bytes, slot, &fresh);
  if (p && fresh) {
    // outside a capture: filled now.  Allocated in the middle of a capture (a caller that never ran eagerly first): the fill
    // becomes a node of that graph in front of the first user — a small memset per replay of that one graph, harmless (every
    // user leaves the counters at zero)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cs);
    const hipError_t err = hipMemsetAsync(p, 0, bytes, st);
    if (err != hipSuccess || (cs == hipStreamCaptureStatusNone && hipStreamSynchronize(st) != hipSuccess)) {
      (void)hipGetLastError();
      return nullptr;
    }
  }
  return p;
}
void gemm_scratch_release() {
  std::lock_guard<std::mutex> lock(g_scratch_mutex);
  for (auto& kv : g_scratch)
    if (kv.second.p) hipFree(kv.second.p);
  g_scratch.clear();
  for (void* p : g_scratch_retired) hipFree(p);
  g_scratch_retired.clear();
}

}  // namespace ns
