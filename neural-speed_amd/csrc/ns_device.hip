// ns_device.hip — the device-backend half of neural-speed's BesTLA surface
// (/root/reference/neural_speed/core/ne_bestla.h:85-112, the set the reference guards with NS_SYCL; reference
// implementation core/layers/ne_bestla_sycl.cpp) for MI355X.  With these symbols a reference tree built with -DNS_SYCL
// runs its UNCHANGED graph device-resident: tensors of the offloaded layers live in HBM (ne_new_device_tensor_impl,
// ne_layers.c:904-1050), BTLA weights are re-laid-out once at load (model_files.h:1515-1527), every operator of those
// layers is a HIP launch on one stream and only the token ids go in and the logits come out over PCIe.
//
// The functions whose signatures are plain pointers are exported under the reference's own names, so libns_hip.so is the
// drop-in for them (the tensor-level functions take ne_tensor and live in glue/ne_bestla_hip_device.c, compiled against the
// reference's headers).  By role (shared: ns_device.h; the host decisions as pure code: ns_device_plan.{h,cpp}):
//   * this file:          device, queue, memory, copy and sync entries; the pool list, the page pre-touch, the copy warm-up
//   * ns_device_load.cpp: the asynchronous weight load path and bestla_device_f32f32_forward
//   * ns_device_ops.hip:  broadcasting add / mul (nd_binary_kernel, dense_binary_kernel) and the lazy norm / silu peephole
//   * ns_device_mha.hip:  attention over the fp32 kv cache: on its fp16 mirror, or mha_f32_split_kernel / mha_f32_kernel
//   * ns_device_kvm.cpp:  the fp16 mirrors of that cache (ns_route.h)
// "queue" is a hipStream_t throughout.
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/ns_bestla.h"
#include "ns_common.h"
#include "ns_device.h"
#include "ns_route.h"

extern "C" {
// The runtime builds its pinned staging for copies from / to pageable host memory under the first such copy (a prompt's embeddings: 24.6 MB in 2.1 ms the
// first time, 0.5 ms afterwards).  One 32 MB round trip at device creation — model-load time — moves that out of the first prompt.
static void warm_pageable_copies(hipStream_t s) {
  static const bool off = getenv("NS_WARM_UP") && atoi(getenv("NS_WARM_UP")) == 0;
  static std::once_flag once;
  if (off) return;
  std::call_once(once, [s] {
    const size_t n = size_t(32) << 20;
    void* d = nullptr;
    char* h = static_cast<char*>(calloc(n, 1));
    if (h && hipMalloc(&d, n) == hipSuccess) {
      (void)hipMemcpyAsync(d, h, n, hipMemcpyDefault, s);
      (void)hipMemcpyAsync(h, d, n, hipMemcpyDefault, s);
      (void)hipStreamSynchronize(s);
    }
    if (d) (void)hipFree(d);
    free(h);
    (void)hipGetLastError();
  });
}
/* ---- ne_bestla.h:86-96, ne_bestla_sycl.cpp:26-92 ---- */
void* bestla_create_device(bool profile) {
  (void)profile;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    ns::set_error("bestla_create_device: no HIP device visible");
    return nullptr;
  }
  ns::Device* d = new ns::Device();
  d->id = 0;
  if (hipGetDevice(&d->id) != hipSuccess || hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) {
    delete d;
    ns::set_error("bestla_create_device: stream creation failed");
    return nullptr;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, d->id) == hipSuccess)
    fprintf(stderr, "bestla device: %s, %d CUs, %.1f GB\n", prop.name, prop.multiProcessorCount, double(prop.totalGlobalMem) / 1e9);
  ns::route_attach(d->stream);  // ns_route.cpp: the per-token graph this queue carries is verified and replayed
  (void)ns_hip_warm_up();       // the code objects of the GEMM / GEMV / attention / operator kernels are loaded here, not under the first prompt and token
  warm_pageable_copies(d->stream);
  return d;
}
void* bestla_get_device_queue(void* device) { return device ? static_cast<ns::Device*>(device)->stream : nullptr; }
void bestla_release_device(void* device) {
  if (!device) return;
  (void)ns_hip_lazy_flush();
  ns::finish_pending_loads_if_any();
  ns::Device* d = static_cast<ns::Device*>(device);
  (void)ns::route_sync_point(d->stream);
  ns::route_invalidate();  // (the mirrors go below: no plan of ANY queue may keep a captured cache write into one)
  ns::route_detach(d->stream);
  ns::kvm_clear();
  (void)hipStreamSynchronize(d->stream);
  (void)hipStreamDestroy(d->stream);
  delete d;
}
size_t bestla_device_gmem_size(void* device) {
  (void)device;
  size_t fr = 0, total = 0;
  return hipMemGetInfo(&fr, &total) == hipSuccess ? total : 0;
}
// the reference's device pools come from here: what lies inside one of these allocations is device memory (no runtime query per copy)
static std::mutex g_pool_mu;
static std::vector<std::pair<const char*, size_t>> g_pools;
static bool in_device_pool(const void* p) {
  const char* c = static_cast<const char*>(p);
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (const auto& a : g_pools)
    if (c >= a.first && c < a.first + a.second) return true;
  return false;
}
void* bestla_device_malloc(size_t size, void* queue) {
  (void)queue;
  void* p = nullptr;
  if (hipMalloc(&p, size ? size : 1) != hipSuccess) {
    ns::set_error("bestla_device_malloc: out of device memory");
    return nullptr;
  }
  std::lock_guard<std::mutex> lk(g_pool_mu);
  g_pools.emplace_back(static_cast<const char*>(p), size ? size : 1);
  return p;
}
void bestla_device_free(void* ptr, void* queue) {
  (void)queue;
  // nothing recorded or in flight may still refer to the memory: the lazy node's operands, the route's window and plans, the kv mirrors,
  // the loads into the graph's slices
  (void)ns_hip_lazy_flush();
  ns::route_invalidate();
  ns::kvm_clear();
  ns::finish_pending_loads_if_any();
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pools.size(); i++)
      if (g_pools[i].first == static_cast<const char*>(ptr)) {
        g_pools.erase(g_pools.begin() + long(i));
        break;
      }
  }
  if (ptr) (void)hipFree(ptr);
}
// (Round 6 measured and did NOT adopt a library-side path for large copies to / from pageable host memory — two pinned 16 MB stages, the DMA of chunk i + 1 under
// the host copy of chunk i, that copy cut over eight threads — for the 192 MB of logits a 1500-token prompt's evaluation ends with (ne_layers.c:8345-8346): the
// runtime's own staged copy is as fast once the destination's pages exist (3.45 vs 3.8 ms) and what a FIRST evaluation pays is the first touch of those pages
// (10-18 ms either way, run to run); towards the device the runtime was faster outright (24.6 MB: 1.3 vs 3.5 ms).  profiles/r06_route_timings.txt.)
// Also measured and not adopted: faulting the destination's pages in by eight threads IN FRONT of the copy (the queue already empty): populate + copy
// 23.6-24.4 ms against 13.9-17.2 ms for the copy alone.  docs/kernels/experiments.md.)
// What IS done: two threads, while the queue still works on what the copy waits for — bestla_device_sync in front of the copy is deferred (ns_route.cpp
// route_defer_sync), so the copy call arrives with the prompt's launches in flight and the host otherwise idle.
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
// The destination of a large copy to pageable host memory, first-touched while the queue still works on what the copy waits for (contents untouched;
// 8 MB at a time, stopping as soon as the queue is empty; anything the call refuses — an older kernel, a special mapping — is left to the copy)
static void touch_destination_while_queue_runs(void* dst, size_t size, hipStream_t s) {
  static const bool off = getenv("NS_DEVICE_PRETOUCH") && atoi(getenv("NS_DEVICE_PRETOUCH")) == 0;
  if (off || size < (size_t(8) << 20)) return;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone || hipStreamQuery(s) != hipErrorNotReady) {  // (a query would end a capture)
    (void)hipGetLastError();
    return;
  }
  hipPointerAttribute_t at;
  const bool known = hipPointerGetAttributes(&at, dst) == hipSuccess && at.type != hipMemoryTypeUnregistered;
  (void)hipGetLastError();
  if (known) return;  // pinned / device / managed: nothing to fault in
  // two threads: 192 MB of fresh pages measured 17-19 ms with one, 9-11 with two, 5-13 with four, 15-16 with eight or sixteen (the GPU boxes' hosts)
  const uintptr_t pg = uintptr_t(sysconf(_SC_PAGESIZE)), step = uintptr_t(8) << 20;
  const uintptr_t lo = (reinterpret_cast<uintptr_t>(dst) + pg - 1) & ~(pg - 1), hi = (reinterpret_cast<uintptr_t>(dst) + size) & ~(pg - 1);
  if (hi <= lo) return;
  const uintptr_t mid = (lo + (hi - lo) / 2) & ~(pg - 1);
  std::atomic<bool> stop{false};
  auto run = [&stop, step](uintptr_t a, uintptr_t e) {
    for (; a < e && !stop.load(std::memory_order_relaxed); a += step)
      if (madvise(reinterpret_cast<void*>(a), size_t(std::min(step, e - a)), MADV_POPULATE_WRITE) != 0) break;
  };
  std::thread helper(run, mid, hi);
  for (uintptr_t a = lo; a < mid; a += step) {
    if (madvise(reinterpret_cast<void*>(a), size_t(std::min(step, mid - a)), MADV_POPULATE_WRITE) != 0) break;
    if (hipStreamQuery(s) != hipErrorNotReady) break;  // the queue is empty: the rest is left to the copy
  }
  stop.store(true);
  helper.join();
  (void)hipGetLastError();
}
static void device_memcpy_impl(void* dstptr, const void* srcptr, size_t size, void* queue, bool wait_first) {
  (void)ns_hip_lazy_flush();
  // what the route holds back (its window) goes out first; a copy FROM device memory reads a tensor behind the window's last op
  const bool from_dev = srcptr && in_device_pool(srcptr);
  (void)ns::route_sync_point(queue, from_dev ? srcptr : nullptr, from_dev ? size : 0);
  if (!dstptr || !srcptr || !size) return;
  if (wait_first && from_dev) {
    (void)hipStreamSynchronize(static_cast<hipStream_t>(queue));
    (void)ns::route_after_sync(queue);
  }
  if (from_dev && !in_device_pool(dstptr)) touch_destination_while_queue_runs(dstptr, size, static_cast<hipStream_t>(queue));
  // (replayed tokens run on the plan's activations: the embeddings go there as well, the logits come from there — ns_route.cpp)
  void* twin = ns::route_twin_dst(dstptr, queue);
  srcptr = ns::route_translate_src(srcptr, queue);
  if (twin && hipMemcpyAsync(twin, srcptr, size, hipMemcpyDefault, static_cast<hipStream_t>(queue)) != hipSuccess)
    ns::set_error("bestla_device_memcpy failed");
  if (hipMemcpyAsync(dstptr, srcptr, size, hipMemcpyDefault, static_cast<hipStream_t>(queue)) != hipSuccess)
    ns::set_error("bestla_device_memcpy failed");
  ns::route_note_copy(queue);
  if (in_device_pool(dstptr)) {
    // a copy into a mirrored kv cache (a restored session, a beam's rows): its mirror starts over, and no plan may go on replaying on the old one.
    // The order matters: plans are dropped first (that leaves every mirror marked up to the last replayed token), THEN the mirror is marked empty
    if (ns::kvm_note_foreign_write(dstptr, size)) {
      ns::route_invalidate();
      (void)ns::kvm_note_foreign_write(dstptr, size);
    }
    ns::route_note_input(dstptr, size, queue);     // an evaluation's input: kept so that the evaluation can be issued again
  }
}
// The exported copy WITHOUT a wait of its own (ne_bestla.h:92): a caller that fetches results with it and bestla_device_sync gets no second chance behind
// the wait — an evaluation that has to be run again (fp16 overflow, ns_route.h) must have been by the time its results are read.  A copy FROM device memory
// therefore waits for the queue and lets the route look at the flag first; towards the device nothing changes.  (bestla_device_memcpy_sync, the reference's
// only form, keeps its order: copy, deferred wait, copy again if need be.)
void bestla_device_memcpy(void* dstptr, const void* srcptr, size_t size, void* queue) { device_memcpy_impl(dstptr, srcptr, size, queue, true); }
static bool device_sync_impl(void* queue) {
  (void)ns_hip_lazy_flush();
  ns::route_time_mark(queue, 0);
  (void)ns::route_sync_point(queue);
  if (ns::route_defer_sync(queue)) return false;  // (only launches in flight: the next copy's wait covers them — ns_route.cpp)
  (void)hipStreamSynchronize(static_cast<hipStream_t>(queue));
  return ns::route_after_sync(queue);
}
void bestla_device_sync(void* queue) { (void)device_sync_impl(queue); }
void bestla_device_memcpy_sync(void* dstptr, const void* srcptr, size_t size, void* queue) {
  static const bool timing = getenv("NS_ROUTE_TIMING") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  device_memcpy_impl(dstptr, srcptr, size, queue, false);
  const bool again = device_sync_impl(queue);
  if (timing && size >= (size_t(8) << 20))
    fprintf(stderr, "route timing: bestla_device_memcpy_sync of %.1f MB took %.2f ms\n", size / 1e6,
            std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() / 1e3);
  if (again) {  // the evaluation this copy reads from was run again (fp16 overflow, ns_route.h): its results are fetched again
    device_memcpy_impl(dstptr, srcptr, size, queue, false);
    (void)hipStreamSynchronize(static_cast<hipStream_t>(queue));
    (void)ns::route_after_sync(queue);
  }
  ns::route_time_mark(queue, 1);
}

}  // extern "C"
