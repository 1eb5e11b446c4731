// ns_host_entry.cpp — the reference's host-pointer surface of libns_hip.so: ns_BTLAGemm* (pack / unpack) and every bestla_* entry.  Each
// one stages its host tensors (pinned zero-copy at decode size, staged copies above), looks its weights up in the cache
// (ns_weights.cpp) and calls the device-pointer entry that serves it (ns_dispatch.cpp).
//
// Mirrors the reference's operator boundary:
//   neural_speed/core/ne_bestla.h:21-83                      (extern "C" surface, part 1)
//   neural_speed/core/layers/inner_product.cpp:20-36         (bestla_f32f32_{get_workspace_size,forward})
//   neural_speed/core/layers/bestla_gemm.cpp:508-749         (BTLAGemmBatchDriver / PackBSize / QuantPackB / PackB / UnPackB)
//   neural_speed/core/layers/ip_fusion_qkv.cpp:155-307, ip_fusion_ffn.cpp:20-29,724-779
//   neural_speed/core/layers/ne_bestla.cpp:19-164
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ns_api_int.h"

using namespace ns;  // NOLINT

namespace {
// The host-pointer entry points share process-wide staging buffers (and the default stream).  The reference runs them
// from one thread at a time (n_tasks = 1, ne_bestla.cpp:270-272); callers that do not are serialised here.
std::mutex g_host_mu;
int g_pack_core = NS_CORE_AUTO;
struct Scratch {  // growable device scratch for the host-pointer API
  void* p = nullptr;
  size_t cap = 0;
  void* get(size_t bytes) {
    if (bytes > cap) {
      if (p) hipFree(p);
      p = nullptr;
      cap = 0;
      if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
      cap = bytes;
    }
    return p;
  }
};
Scratch g_sa, g_sc, g_st1, g_st2, g_sd;

// Pinned, device-mapped host staging for the small-M host-pointer calls: the kernel reads A from and writes C to host
// memory over PCIe directly (a few KB), so a call is memcpy + ONE launch + ONE synchronisation instead of three blocking
// hipMemcpy round trips (measured 133 us -> see DESIGN.md for a 4096 -> 11008 GEMV).
struct PinnedScratch {
  void* p = nullptr;
  size_t cap = 0;
  void* get(size_t bytes) {
    if (bytes > cap) {
      if (p) hipHostFree(p);
      p = nullptr;
      cap = 0;
      const size_t want = bytes < (size_t(1) << 16) ? (size_t(1) << 16) : bytes;
      if (hipHostMalloc(&p, want, hipHostMallocMapped) != hipSuccess) {
        p = nullptr;
        return nullptr;
      }
      cap = want;
    }
    return p;
  }
};
PinnedScratch g_ha, g_hc, g_hd, g_ht1, g_ht2;
Scratch g_s16;  // device fp16 shadow of the FFN intermediate on the zero-copy path
constexpr size_t kZeroCopyMaxBytes = size_t(2) << 20;  // beyond this the staged-copy path wins
inline float* mapped(PinnedScratch& s, size_t bytes, float** host) {
  *host = static_cast<float*>(s.get(bytes));
  void* d = nullptr;
  if (!*host || hipHostGetDevicePointer(&d, *host, 0) != hipSuccess) return nullptr;
  return static_cast<float*>(d);
}
inline bool zero_copy_enabled() {
  static const bool off = getenv("NS_NO_ZERO_COPY") != nullptr;  // diagnostics
  return !off;
}

void invalid_parameters(const char* who) {  // inner_product.cpp:31-35 (release build: print and carry on)
  printf("Err: invalid parameters (%s: %s)\n", who, ns_hip_last_error());
}

struct PackPlan {
  BlobView v;
  int core;
};
bool plan_pack(PackPlan* pp, size_t N, size_t K, size_t BlkSize, uint32_t qt, uint32_t st, bool asym, int comp,
               uintptr_t base_addr, bool shuffle = false) {
  const size_t bs_eff = (int64_t(BlkSize) <= 0) ? K : BlkSize;
  pp->core = core_for_comp(comp, qt, asym, bs_eff, g_pack_core);
  const CoreDesc& cd = core_desc(pp->core);
  if (bs_eff % cd.ktile != 0 && int64_t(BlkSize) > 0) {
    set_error("pack: block size is not a multiple of the target core's KTILE");
    return false;
  }
  std::string err;
  // shuffle indices exist for integer weights only (BTLAGemmPackBImpl, bestla_gemm.cpp:407-419)
  if (!blob_describe(&pp->v, N, K, BlkSize, qt, st, asym, pp->core, base_addr, &err, shuffle && dt_is_int(qt))) {
    set_error(err);
    return false;
  }
  return true;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------------ part 2
void ns_set_pack_core(int core) { g_pack_core = core; }

size_t ns_BTLAGemmPackBSize(size_t N, size_t K, size_t BlkSize, uint32_t QuantType, uint32_t ScaleDtype, bool isAsym,
                            int CompType, int* shuffle_indice) {
  PackPlan pp;
  if (!plan_pack(&pp, N, K, BlkSize, QuantType, ScaleDtype, isAsym, CompType, 0, shuffle_indice != nullptr)) return 0;
  return pp.v.size;
}

static bool pack_common(void* PackedBuf, const float* FpData, const int8_t* QData, const float* Scales,
                        const int8_t* Zp, size_t N, size_t K, size_t ldb, size_t BlkSize, uint32_t qt, uint32_t stp,
                        bool asym, int comp, bool isTrans, const int* g_idx = nullptr) {
  if (!have_device()) return false;
  PackPlan pp;
  if (!plan_pack(&pp, N, K, BlkSize, qt, stp, asym, comp, reinterpret_cast<uintptr_t>(PackedBuf), g_idx != nullptr))
    return false;
  std::vector<int> idx;
  if (g_idx) {
    // setShuffleIndices (bestla_prologue_b.h:337-356): slot g * blocksize + (members of group g seen so far) <- k.
    // K ints of index bookkeeping on the host; the codes arrive already sorted this way (convert/common.py:667-681).
    const size_t bs = size_t(pp.v.blocksize), groups = (K + bs - 1) / bs;
    std::vector<int> count(groups, 0);
    idx.assign(K, 0);
    for (size_t i = 0; i < K; i++) {
      const int g = g_idx[i];
      if (g < 0 || size_t(g) >= groups || size_t(g) * bs + size_t(count[g]) >= K) {
        set_error("pack: g_idx does not describe groups of `BlkSize` input channels");
        return false;
      }
      idx[size_t(g) * bs + size_t(count[g]++)] = int(i);
    }
  }
  const BlobView& v = pp.v;
  uint8_t* host = static_cast<uint8_t*>(PackedBuf);
  blob_write_header(v, host);  // == stor.assign(PackedBuf), bestla_gemm.cpp:312
  if (g_idx) memcpy(host + v.shuf_off, idx.data(), K * sizeof(int));
  DevBuf<uint8_t> dq, ds;
  DevBuf<int8_t> dz;
  DevBuf<uint16_t> dr;
  if (!dq.alloc(v.q_bytes) || !ds.alloc(v.s_bytes)) return false;
  if (v.asym() && !dz.alloc(v.z_bytes)) return false;
  if (v.has_reduce() && !dr.alloc(v.r_bytes / 2)) return false;
  hipStream_t st = nullptr;
  hipError_t e;
  if (FpData) {
    const size_t rows = isTrans ? N : K, cols = isTrans ? K : N;
    DevBuf<float> dw;
    if (!dw.alloc(rows * cols)) return false;
    if (!hip_ok(hipMemcpy2D(dw.p, cols * 4, FpData, ldb * 4, cols * 4, rows, hipMemcpyHostToDevice), "H2D weight"))
      return false;
    QuantArgs qa{dw.p, N, K, cols, isTrans, v.blocksize, qt, stp, v.asym(), v.ntile(), v.packrow(), v.kpad, v.npad,
                 v.cstep, v.has_reduce(), dq.p, ds.p, dz.p, dr.p};
    e = launch_quant_pack(qa, st);
    if (!hip_ok(e, "quant_pack") || !hip_ok(hipStreamSynchronize(st), "quant_pack sync")) return false;
  } else {
    const size_t nblk = (K + v.blocksize - 1) / v.blocksize;
    DevBuf<int8_t> q, z;
    DevBuf<float> s;
    if (!q.alloc(N * K) || !s.alloc(nblk * N)) return false;
    if (!hip_ok(hipMemcpy2D(q.p, N, QData, ldb, N, K, hipMemcpyHostToDevice), "H2D codes")) return false;
    if (!hip_ok(hipMemcpy(s.p, Scales, nblk * N * 4, hipMemcpyHostToDevice), "H2D scales")) return false;
    if (asym) {
      if (!z.alloc(nblk * N)) return false;
      if (!hip_ok(hipMemcpy(z.p, Zp, nblk * N, hipMemcpyHostToDevice), "H2D zps")) return false;
    }
    PackQArgs pa{q.p, s.p, asym ? z.p : nullptr, N, K, N, v.blocksize, qt, stp, v.ntile(), v.packrow(), v.kpad, v.npad,
                 v.cstep, v.has_reduce(), dq.p, ds.p, dz.p, dr.p};
    e = launch_pack_q(pa, st);
    if (!hip_ok(e, "pack_q") || !hip_ok(hipStreamSynchronize(st), "pack_q sync")) return false;
  }
  if (!hip_ok(hipMemcpy(host + v.q_off, dq.p, v.q_bytes, hipMemcpyDeviceToHost), "D2H codes")) return false;
  if (!hip_ok(hipMemcpy(host + v.s_off, ds.p, v.s_bytes, hipMemcpyDeviceToHost), "D2H scales")) return false;
  if (v.asym() && !hip_ok(hipMemcpy(host + v.z_off, dz.p, v.z_bytes, hipMemcpyDeviceToHost), "D2H zps")) return false;
  if (v.has_reduce()) {
    // the reference leaves padded columns / rows of the reduce buffer untouched (prologue_b.h:455-470): copy only
    // what reduceWeight writes.
    const size_t nblk = (K + v.blocksize - 1) / v.blocksize;
    if (!hip_ok(hipMemcpy2D(host + v.r_off, size_t(v.cstep) * 2, dr.p, size_t(v.cstep) * 2, N * 2, nblk,
                            hipMemcpyDeviceToHost),
                "D2H reduce"))
      return false;
  }
  return true;
}

// the same quantizer on a weight and a blob that live in device memory
int ns_hip_quant_pack_device(void* dBlob, const float* dW, size_t N, size_t K, size_t ldb, size_t BlkSize,
                             uint32_t QuantType, uint32_t ScaleDtype, bool isAsym, int CompType, bool isTrans,
                             void* stream) {
  if (!have_device()) return -1;
  hipStream_t st = (hipStream_t)stream;
  PackPlan pp;
  if (!plan_pack(&pp, N, K, BlkSize, QuantType, ScaleDtype, isAsym, CompType, reinterpret_cast<uintptr_t>(dBlob)))
    return -1;
  uint8_t* base = static_cast<uint8_t*>(dBlob);
  const BlobView& v = pp.v;
  bool io_ok = true;
  BlobIo io = [&](size_t off, void* buf, size_t n, bool) {
    if (hipMemcpyAsync(base + off, buf, n, hipMemcpyHostToDevice, st) != hipSuccess) io_ok = false;
    hipStreamSynchronize(st);  // `buf` is a stack temporary
  };
  blob_write_header_io(v, io, reinterpret_cast<uintptr_t>(dBlob));
  if (!io_ok) {
    set_error("quant_pack_device: header write failed");
    return -1;
  }
  QuantArgs qa{dW, N, K, ldb, isTrans, v.blocksize, QuantType, ScaleDtype, v.asym(), v.ntile(), v.packrow(), v.kpad,
               v.npad, v.cstep, v.has_reduce(), base + v.q_off, base + v.s_off,
               v.asym() ? (int8_t*)(base + v.z_off) : nullptr, v.has_reduce() ? (uint16_t*)(base + v.r_off) : nullptr};
  return hip_ok(launch_quant_pack(qa, st), "quant_pack") ? 0 : -1;
}

bool ns_BTLAGemmQuantPackB(void* PackedBuf, const float* FpData, size_t N, size_t K, size_t ldb, size_t BlkSize,
                           uint32_t QuantType, uint32_t ScaleDtype, bool isAsym, int CompType, bool isTrans,
                           void* ThreadPool) {
  (void)ThreadPool;
  return pack_common(PackedBuf, FpData, nullptr, nullptr, nullptr, N, K, ldb, BlkSize, QuantType, ScaleDtype, isAsym,
                     CompType, isTrans);
}

bool ns_BTLAGemmPackB(void* PackedBuf, const int8_t* QData, const float* Scales, const int8_t* Zp, size_t N, size_t K,
                      size_t ldb, size_t BlkSize, uint32_t QuantType, uint32_t ScaleDtype, bool isAsym, int CompType,
                      int* shuffle_indice, void* ThreadPool) {
  (void)ThreadPool;
  if (!dt_is_int(QuantType)) return false;  // bestla_gemm.cpp:431-433
  return pack_common(PackedBuf, nullptr, QData, Scales, isAsym ? Zp : nullptr, N, K, ldb, BlkSize, QuantType,
                     ScaleDtype, isAsym, CompType, false, shuffle_indice);
}

bool ns_BTLAGemmUnPackB(float* FpData, const void* PackedBuf, size_t N, size_t K, size_t ldb, void* ThreadPool) {
  (void)ThreadPool;
  CachePin pin;
  ns_weight* w = cached_weight(PackedBuf);
  if (!w) return false;
  if (size_t(w->n) != N || size_t(w->k) != K) {
    set_error("unpack: shape mismatch");
    return false;
  }
  DevBuf<float> d;
  if (!d.alloc(N * K)) return false;
  if (!hip_ok(launch_unpack_fp32(w, d.p, int(N), nullptr), "unpack")) return false;
  return hip_ok(hipMemcpy2D(FpData, ldb * 4, d.p, N * 4, N * 4, K, hipMemcpyDeviceToHost), "D2H unpack");
}

// ------------------------------------------------------------------------------------------------ part 1
void bestla_init(void) {
  int c = ns_hip_device_count();
  if (c <= 0) {
    printf("libns_hip: no HIP device visible\n");
    return;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) == hipSuccess)
    printf("libns_hip: %d device(s), device 0 = %s (%s), %d CUs, %.0f GB\n", c, prop.name, prop.gcnArchName,
           prop.multiProcessorCount, double(prop.totalGlobalMem) / 1e9);
}

void bestla_timer(bool _init) {
  static std::chrono::steady_clock::time_point t0;
  if (_init)
    t0 = std::chrono::steady_clock::now();
  else
    printf("time :%f us\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
}

int bestla_set_threads(int _nth) { return _nth; }

void* bestla_get_thread_handle(void) { return &g_host_mu; }  // (opaque and non-null; the reference hands out its thread pool)

unsigned long long bestla_f32f32_get_workspace_size(int _m, int _n, int _k, void* wptr) {
  (void)_n;
  (void)wptr;
  // keep the reference's host-workspace contract (inner_product.cpp:20-25) so callers size buffers identically;
  // the device path does not use the host workspace.
  const size_t kp = (size_t(_k) + 127) / 128 * 128;
  return size_t(_m) * kp * 4;
}

static bool host_forward(float* activation, void* weiptr, float* output, int m, int n, int k, int lda, int ldo,
                         int epi, const float* hostD, int ldd_rows, int ldd) {
  std::lock_guard<std::mutex> host_lock(g_host_mu);
  CachePin pin;
  ns_weight* w = cached_weight(weiptr);
  if (!w) return false;
  if (w->n != n || w->k != k) {
    set_error("forward: blob shape does not match (n, k)");
    return false;
  }
  const size_t bytes_a = size_t(m) * k * 4, bytes_c = size_t(m) * n * 4, bytes_d = hostD ? size_t(ldd_rows) * n * 4 : 0;
  if (zero_copy_enabled() && m <= 64 && bytes_a + bytes_c + bytes_d <= kZeroCopyMaxBytes) {
    float* hA = (float*)g_ha.get(bytes_a);
    float* hC = (float*)g_hc.get(bytes_c);
    float* hD = hostD ? (float*)g_hd.get(bytes_d) : nullptr;
    void *dAz = nullptr, *dCz = nullptr, *dDz = nullptr;
    if (hA && hC && (!hostD || hD) && hipHostGetDevicePointer(&dAz, hA, 0) == hipSuccess &&
        hipHostGetDevicePointer(&dCz, hC, 0) == hipSuccess && (!hostD || hipHostGetDevicePointer(&dDz, hD, 0) == hipSuccess)) {
      for (int r = 0; r < m; r++) memcpy(hA + size_t(r) * k, activation + size_t(r) * lda, size_t(k) * 4);
      int dldd = 0;
      if (hostD) {
        for (int r = 0; r < ldd_rows; r++) memcpy(hD + size_t(r) * n, hostD + size_t(r) * (ldd ? ldd : n), size_t(n) * 4);
        dldd = ldd ? n : 0;
      }
      if (forward_impl((const float*)dAz, w, (float*)dCz, m, k, n, epi, (const float*)dDz, dldd, nullptr)) return false;
      if (!hip_ok(hipStreamSynchronize(nullptr), "synchronize")) return false;
      for (int r = 0; r < m; r++) memcpy(output + size_t(r) * ldo, hC + size_t(r) * n, size_t(n) * 4);
      return true;
    }
    (void)hipGetLastError();  // pinned allocation refused: fall through to the staged copies
  }
  float* dA = (float*)g_sa.get(bytes_a);
  float* dC = (float*)g_sc.get(bytes_c);
  if (!dA || !dC) {
    set_error("forward: device scratch allocation failed");
    return false;
  }
  if (!hip_ok(hipMemcpy2D(dA, size_t(k) * 4, activation, size_t(lda) * 4, size_t(k) * 4, m, hipMemcpyHostToDevice), "H2D A"))
    return false;
  float* dD = nullptr;
  int dldd = 0;
  if (hostD) {
    dD = (float*)g_sd.get(size_t(ldd_rows) * n * 4);
    if (!dD) return false;
    if (!hip_ok(hipMemcpy2D(dD, size_t(n) * 4, hostD, size_t(ldd ? ldd : n) * 4, size_t(n) * 4, ldd_rows, hipMemcpyHostToDevice),
                "H2D D"))
      return false;
    dldd = ldd ? n : 0;
  }
  if (forward_impl(dA, w, dC, m, k, n, epi, dD, dldd, nullptr)) return false;
  return hip_ok(hipMemcpy2D(output, size_t(ldo) * 4, dC, size_t(n) * 4, size_t(n) * 4, m, hipMemcpyDeviceToHost), "D2H C");
}

void bestla_f32f32_forward(float* activation, void* weiptr, float* output, int _m, int _n, int _k, int lda, int ldo,
                           void* workspace) {
  ns::HostScope host_scope("bestla_f32f32_forward");
  (void)workspace;
  if (!have_device() || !host_forward(activation, weiptr, output, _m, _n, _k, lda, ldo, NS_EPI_NONE, nullptr, 0, 0))
    invalid_parameters("bestla_f32f32_forward");
}

// The reference's model code asks these for every layer of every evaluation (llama.cpp:212, :609).  On its device route a weight tensor's data is the
// storage record of bestla_device_load_storage, not a blob (first word all ones: no blob starts like that, csrc/ns_device.h DeviceStorage) — refused
// here as the parse would refuse it, without the lock, the cache lookup and the error text: the unfused nodes the reference then builds are the ones its
// own device branch builds (ne_bestla.cpp:222-225).
static inline bool is_device_record(const void* p) {
  uint64_t v = 0;
  if (p) memcpy(&v, p, 8);
  return v == ~uint64_t(0);
}
bool bestla_fusion_add_f32f32_support(void* weiptr, int _m, int _n, int _k) {
  (void)_m;
  if (is_device_record(weiptr)) return false;
  if (ns_hip_device_count() <= 0) return false;
  std::lock_guard<std::mutex> host_lock(g_host_mu);
  CachePin pin;
  ns_weight* w = cached_weight(weiptr);
  return w && w->n == _n && w->k == _k;
}

void bestla_fusion_add_f32f32_forward(float* activation, void* weiptr, float* bias, float* output, int _m, int _n,
                                      int _k, int lda, int ldo, bool boardcast_bias, void* workspace) {
  ns::HostScope host_scope("bestla_fusion_add_f32f32_forward");
  (void)workspace;
  // custom::epilogue::Add with ldd = broadcast ? 0 : ldo (inner_product.cpp:113-244)
  if (!have_device() || !host_forward(activation, weiptr, output, _m, _n, _k, lda, ldo, NS_EPI_ADD, bias,
                                      boardcast_bias ? 1 : _m, boardcast_bias ? 0 : ldo))
    invalid_parameters("bestla_fusion_add_f32f32_forward");
}

unsigned long long bestla_fusion_QKV_f32f32_get_workspace_size(int _m, int _n, int _k, void* w1ptr) {
  return bestla_f32f32_get_workspace_size(_m, _n, _k, w1ptr);  // ip_fusion_qkv.cpp:155-161
}

bool bestla_fusion_QKV_f32f32_support(void* wqptr, void* wkptr, void* wvptr, int _m, int _n, int _k) {
  (void)_m;
  if (is_device_record(wqptr) || is_device_record(wkptr) || is_device_record(wvptr)) return false;
  if (ns_hip_device_count() <= 0) return false;
  std::lock_guard<std::mutex> host_lock(g_host_mu);
  CachePin pin;
  ns_weight *q = cached_weight(wqptr), *k = cached_weight(wkptr), *v = cached_weight(wvptr);
  if (!q || !k || !v) return false;
  if (q->shuf || k->shuf || v->shuf) return false;  // ip_fusion_qkv.cpp:174-176: no QKV fusion with activation shuffle
  // samePackedWeight (bestla_common.hpp:90-119): identical shape + format for all three
  for (ns_weight* w : {q, k, v})
    if (w->n != _n || w->k != _k || !same_quant(w, q)) return false;
  return true;
}

void bestla_fusion_QKV_f32f32_forward(float* activation, void* wqptr, void* wkptr, void* wvptr, float* output, int _m,
                                      int _n, int _k, int lda, int ldo, void* workspace) {
  ns::HostScope host_scope("bestla_fusion_QKV_f32f32_forward");
  std::lock_guard<std::mutex> host_lock(g_host_mu);
  CachePin pin;
  (void)workspace;
  bool ok = have_device();
  ns_weight *q = nullptr, *k = nullptr, *v = nullptr;
  if (ok) {
    q = cached_weight(wqptr);
    k = cached_weight(wkptr);
    v = cached_weight(wvptr);
    ok = q && k && v;
  }
  if (ok && zero_copy_enabled() && _m <= 64 && size_t(_m) * (size_t(_k) + 3 * size_t(_n)) * 4 <= kZeroCopyMaxBytes) {
    // small M: A read from / QKV written to pinned device-mapped host memory, one launch + one synchronisation
    float *hA = nullptr, *hC = nullptr;
    float* dA = mapped(g_ha, size_t(_m) * _k * 4, &hA);
    float* dC = mapped(g_hc, size_t(3) * _m * _n * 4, &hC);
    if (dA && dC) {
      for (int r = 0; r < _m; r++) memcpy(hA + size_t(r) * _k, activation + size_t(r) * lda, size_t(_k) * 4);
      ok = ns_hip_fusion_qkv_forward(dA, q, k, v, dC, _m, _k, _n, nullptr) == 0 && hip_ok(hipStreamSynchronize(nullptr), "synchronize");
      if (ok)
        for (int r = 0; r < 3 * _m; r++) memcpy(output + size_t(r) * ldo, hC + size_t(r) * _n, size_t(_n) * 4);
      if (!ok) invalid_parameters("bestla_fusion_QKV_f32f32_forward");
      return;
    }
    (void)hipGetLastError();
  }
  if (ok) {
    float* dA = (float*)g_sa.get(size_t(_m) * _k * 4);
    float* dC = (float*)g_sc.get(size_t(3) * _m * _n * 4);
    ok = dA && dC &&
         hip_ok(hipMemcpy2D(dA, size_t(_k) * 4, activation, size_t(lda) * 4, size_t(_k) * 4, _m, hipMemcpyHostToDevice), "H2D A") &&
         ns_hip_fusion_qkv_forward(dA, q, k, v, dC, _m, _k, _n, nullptr) == 0 &&
         hip_ok(hipMemcpy2D(output, size_t(ldo) * 4, dC, size_t(_n) * 4, size_t(_n) * 4, size_t(3) * _m, hipMemcpyDeviceToHost), "D2H C");
  }
  if (!ok) invalid_parameters("bestla_fusion_QKV_f32f32_forward");
}

unsigned long long bestla_fusion_FFN_f32f32_get_workspace_size(int seq, int fin, int fmid, int fout, void* w1ptr,
                                                               void* w2ptr) {
  (void)fout;
  (void)w1ptr;
  (void)w2ptr;
  auto pad = [](size_t x) { return (x + 127) / 128 * 128; };  // ip_fusion_ffn.cpp:20-29
  return size_t(seq) * pad(fin) * 4 + size_t(seq) * pad(fmid) * 4;
}

static bool ffn3_support(void* w1ptr, void* w2ptr, void* w3ptr, int fin, int fmid, int fout) {
  if (is_device_record(w1ptr) || is_device_record(w2ptr) || is_device_record(w3ptr)) return false;
  if (ns_hip_device_count() <= 0) return false;
  std::lock_guard<std::mutex> host_lock(g_host_mu);
  CachePin pin;
  ns_weight *w1 = cached_weight(w1ptr), *w2 = cached_weight(w2ptr), *w3 = cached_weight(w3ptr);
  if (!w1 || !w2 || !w3) return false;
  // (as found: the code type, qtype, is not compared here, unlike same_quant() — left as it is, not harmonised)
  return w1->k == fin && w1->n == fmid && w3->k == fin && w3->n == fmid && w2->k == fmid && w2->n == fout &&
         w1->kind == w3->kind && w1->blocksize == w3->blocksize && w1->scale_dt == w3->scale_dt && w1->asym == w3->asym;
}

static void ffn3_forward(const char* who, float* activation, void* w1ptr, void* w2ptr, void* w3ptr, float* tmp1,
                         float* tmp2, float* output, int seq, int fin, int fmid, int fout, int act) {
  std::lock_guard<std::mutex> host_lock(g_host_mu);
  CachePin pin;
  bool ok = have_device();
  ns_weight *w1 = nullptr, *w2 = nullptr, *w3 = nullptr;
  if (ok) {
    w1 = cached_weight(w1ptr);
    w2 = cached_weight(w2ptr);
    w3 = cached_weight(w3ptr);
    ok = w1 && w2 && w3;
  }
  if (ok && zero_copy_enabled() && smallm_dual_ok(seq) &&
      size_t(seq) * (size_t(fin) + 2 * size_t(fmid) + size_t(fout)) * 4 <= kZeroCopyMaxBytes) {
    // small M: every host-visible tensor lives in pinned device-mapped memory; the down projection reads the fp16
    // shadow of tmp2 that the gate/up epilogue leaves in HBM, so nothing but A crosses PCIe towards the GPU
    float *hA = nullptr, *hT1 = nullptr, *hT2 = nullptr, *hO = nullptr;
    float* dA = mapped(g_ha, size_t(seq) * fin * 4, &hA);
    float* dT1 = mapped(g_ht1, size_t(seq) * fmid * 4, &hT1);
    float* dT2 = mapped(g_ht2, size_t(seq) * fmid * 4, &hT2);
    float* dO = mapped(g_hc, size_t(seq) * fout * 4, &hO);
    void* d16 = g_s16.get(size_t(seq) * fmid * 2);
    if (dA && dT1 && dT2 && dO && d16 && (fmid & 7) == 0) {
      memcpy(hA, activation, size_t(seq) * fin * 4);
      ok = ns_hip_fusion_ffn3_forward_h(dA, nullptr, w1, w2, w3, dT1, dT2, d16, dO, nullptr, seq, act, nullptr) == 0 &&
           hip_ok(hipStreamSynchronize(nullptr), "synchronize");
      if (ok) {
        memcpy(output, hO, size_t(seq) * fout * 4);
        if (tmp1) memcpy(tmp1, hT1, size_t(seq) * fmid * 4);
        if (tmp2) memcpy(tmp2, hT2, size_t(seq) * fmid * 4);
      }
      if (!ok) invalid_parameters(who);
      return;
    }
    (void)hipGetLastError();
  }
  if (ok) {
    float* dA = (float*)g_sa.get(size_t(seq) * fin * 4);
    float* dT1 = (float*)g_st1.get(size_t(seq) * fmid * 4);
    float* dT2 = (float*)g_st2.get(size_t(seq) * fmid * 4);
    float* dO = (float*)g_sc.get(size_t(seq) * fout * 4);
    ok = dA && dT1 && dT2 && dO &&
         hip_ok(hipMemcpy(dA, activation, size_t(seq) * fin * 4, hipMemcpyHostToDevice), "H2D A") &&
         ns_hip_fusion_ffn3_forward(dA, w1, w2, w3, dT1, dT2, dO, seq, act, nullptr) == 0 &&
         hip_ok(hipMemcpy(output, dO, size_t(seq) * fout * 4, hipMemcpyDeviceToHost), "D2H out");
    // the reference leaves act(A*W1) in tmp1 and (A*W3)*tmp1 in tmp2 (graph-allocated temporaries, ne_layers.c:2573-2576)
    if (ok && tmp1) ok = hip_ok(hipMemcpy(tmp1, dT1, size_t(seq) * fmid * 4, hipMemcpyDeviceToHost), "D2H tmp1");
    if (ok && tmp2) ok = hip_ok(hipMemcpy(tmp2, dT2, size_t(seq) * fmid * 4, hipMemcpyDeviceToHost), "D2H tmp2");
  }
  if (!ok) invalid_parameters(who);
}

bool bestla_fusion_FFN_SiLu_f32f32_support(void* w1ptr, void* w2ptr, void* w3ptr, int seq, int fin, int fmid, int fout) {
  (void)seq;
  return ffn3_support(w1ptr, w2ptr, w3ptr, fin, fmid, fout);
}
void bestla_fusion_FFN_SiLu_f32f32_forward(float* activation, void* w1ptr, void* w2ptr, void* w3ptr, float* tmp1,
                                           float* tmp2, float* output, int seq, int fin, int fmid, int fout,
                                           void* workspace) {
  ns::HostScope host_scope("bestla_fusion_FFN_SiLu_f32f32_forward");
  (void)workspace;
  ffn3_forward("bestla_fusion_FFN_SiLu_f32f32_forward", activation, w1ptr, w2ptr, w3ptr, tmp1, tmp2, output, seq, fin,
               fmid, fout, NS_EPI_SILU);
}
bool bestla_fusion_FFN_Gelu_Mul_f32f32_support(void* w1ptr, void* w2ptr, void* w3ptr, int seq, int fin, int fmid,
                                               int fout) {
  (void)seq;
  return ffn3_support(w1ptr, w2ptr, w3ptr, fin, fmid, fout);
}
void bestla_fusion_FFN_Gelu_Mul_f32f32_forward(float* activation, void* w1ptr, void* w2ptr, void* w3ptr, float* tmp1,
                                               float* tmp2, float* output, int seq, int fin, int fmid, int fout,
                                               void* workspace) {
  ns::HostScope host_scope("bestla_fusion_FFN_Gelu_Mul_f32f32_forward");
  (void)workspace;
  ffn3_forward("bestla_fusion_FFN_Gelu_Mul_f32f32_forward", activation, w1ptr, w2ptr, w3ptr, tmp1, tmp2, output, seq,
               fin, fmid, fout, NS_EPI_GELU);
}

static bool ffn2_support(void* w1ptr, void* w2ptr, int fin, int fmid, int fout) {
  if (is_device_record(w1ptr) || is_device_record(w2ptr)) return false;
  if (ns_hip_device_count() <= 0) return false;
  std::lock_guard<std::mutex> host_lock(g_host_mu);
  CachePin pin;
  ns_weight *w1 = cached_weight(w1ptr), *w2 = cached_weight(w2ptr);
  return w1 && w2 && w1->k == fin && w1->n == fmid && w2->k == fmid && w2->n == fout;
}
static void ffn2_forward(const char* who, float* activation, void* w1ptr, void* w2ptr, float* b1, float* b2,
                         float* tmp1, float* output, int seq, int fin, int fmid, int fout, bool bcast) {
  std::lock_guard<std::mutex> host_lock(g_host_mu);
  CachePin pin;
  bool ok = have_device();
  ns_weight *w1 = nullptr, *w2 = nullptr;
  if (ok) {
    w1 = cached_weight(w1ptr);
    w2 = cached_weight(w2ptr);
    ok = w1 && w2;
  }
  if (ok) {
    float* dA = (float*)g_sa.get(size_t(seq) * fin * 4);
    float* dT1 = (float*)g_st1.get(size_t(seq) * fmid * 4);
    float* dO = (float*)g_sc.get(size_t(seq) * fout * 4);
    const size_t brows = bcast ? 1 : seq;
    float* dB = nullptr;
    ok = dA && dT1 && dO;
    if (ok && b1) {
      dB = (float*)g_sd.get(brows * (size_t(fmid) + fout) * 4);
      ok = dB && hip_ok(hipMemcpy(dB, b1, brows * fmid * 4, hipMemcpyHostToDevice), "H2D b1") &&
           hip_ok(hipMemcpy(dB + brows * fmid, b2, brows * fout * 4, hipMemcpyHostToDevice), "H2D b2");
    }
    ok = ok && hip_ok(hipMemcpy(dA, activation, size_t(seq) * fin * 4, hipMemcpyHostToDevice), "H2D A") &&
         ns_hip_fusion_ffn2_forward(dA, w1, w2, dB, dB ? dB + brows * fmid : nullptr, dT1, dO, seq, bcast, nullptr) == 0 &&
         hip_ok(hipMemcpy(output, dO, size_t(seq) * fout * 4, hipMemcpyDeviceToHost), "D2H out");
    if (ok && tmp1) ok = hip_ok(hipMemcpy(tmp1, dT1, size_t(seq) * fmid * 4, hipMemcpyDeviceToHost), "D2H tmp1");
  }
  if (!ok) invalid_parameters(who);
}
bool bestla_fusion_FFN_GeLu_f32f32_support(void* w1ptr, void* w2ptr, int seq, int fin, int fmid, int fout) {
  (void)seq;
  return ffn2_support(w1ptr, w2ptr, fin, fmid, fout);
}
void bestla_fusion_FFN_GeLu_f32f32_forward(float* activation, void* w1ptr, void* w2ptr, float* tmp1, float* output,
                                           int seq, int fin, int fmid, int fout, void* workspace) {
  ns::HostScope host_scope("bestla_fusion_FFN_GeLu_f32f32_forward");
  (void)workspace;
  ffn2_forward("bestla_fusion_FFN_GeLu_f32f32_forward", activation, w1ptr, w2ptr, nullptr, nullptr, tmp1, output, seq,
               fin, fmid, fout, false);
}
bool bestla_fusion_FFN_Add_GeLu_f32f32_support(void* w1ptr, void* w2ptr, int seq, int fin, int fmid, int fout) {
  (void)seq;
  return ffn2_support(w1ptr, w2ptr, fin, fmid, fout);
}
void bestla_fusion_FFN_Add_GeLu_f32f32_forward(float* activation, void* w1ptr, void* w2ptr, float* b1ptr, float* b2ptr,
                                               float* tmp1, float* output, int seq, int fin, int fmid, int fout,
                                               bool boardcast_bias, void* workspace) {
  ns::HostScope host_scope("bestla_fusion_FFN_Add_GeLu_f32f32_forward");
  (void)workspace;
  ffn2_forward("bestla_fusion_FFN_Add_GeLu_f32f32_forward", activation, w1ptr, w2ptr, b1ptr, b2ptr, tmp1, output, seq,
               fin, fmid, fout, boardcast_bias);
}

void bestla_unpackweight_fp32(void* wptr, int n, int k, float* fp32data, int ld) {
  if (!ns_BTLAGemmUnPackB(fp32data, wptr, size_t(n), size_t(k), size_t(ld), nullptr))
    invalid_parameters("bestla_unpackweight_fp32");
}

void bestla_packweight_copyattr(const float* f32ptr, void* dstpr, int n, int k, int ld, void* srcptr) {
  // ne_bestla.cpp:79-111: re-quantize f32ptr ([K][N], ld) with the attributes of the blob at srcptr
  BlobView v;
  std::string err;
  if (!blob_parse(srcptr, &v, &err)) {
    set_error(err);
    invalid_parameters("bestla_packweight_copyattr");
    return;
  }
  int core = -1;
  for (int c = 0; c <= 8; c++)
    if (core_desc(c).id() == v.core_id) core = c;
  const int saved = g_pack_core;
  if (core >= 0) g_pack_core = core;
  const int btype = (v.comp() >> 4) & 0xf;
  const int comp = btype == 1 ? NS_COMP_BF16 : (btype == 3 ? NS_COMP_INT8 : (btype == 0 ? NS_COMP_F32 : NS_COMP_UNDEF));
  const bool ok = ns_BTLAGemmQuantPackB(dstpr, f32ptr, size_t(n), size_t(k), size_t(ld), size_t(v.blocksize), v.dtype,
                                        v.scale_dt, v.asym(), comp, false, nullptr);
  g_pack_core = saved;
  if (!ok) invalid_parameters("bestla_packweight_copyattr");
}

static bool host_unary(size_t in_elems, size_t out_elems, const float* in, float* out,
                       const std::function<hipError_t(const float*, float*)>& fn) {
  if (!in_elems && !out_elems) return true;  // nothing to do (a scratch buffer of zero bytes that was never allocated is a null pointer)
  // decode-sized tensors: pinned, device-mapped staging — memcpy, ONE launch that reads / writes host memory over PCIe, ONE
  // synchronisation (three blocking hipMemcpy round trips cost 36-53 us per call; the graph issues six such calls per layer)
  if (zero_copy_enabled() && (in_elems + out_elems) * 4 <= kZeroCopyMaxBytes) {
    float *hI = nullptr, *hO = nullptr;
    float* dI = mapped(g_ha, in_elems * 4, &hI);
    float* dO = mapped(g_hc, out_elems * 4, &hO);
    if (dI && dO) {
      memcpy(hI, in, in_elems * 4);
      if (!hip_ok(fn(dI, dO), "launch") || !hip_ok(hipStreamSynchronize(nullptr), "synchronize")) return false;
      memcpy(out, hO, out_elems * 4);
      return true;
    }
    (void)hipGetLastError();  // pinned allocation refused: staged copies
  }
  float* dI = (float*)g_sa.get(in_elems * 4);
  float* dO = (float*)g_sc.get(out_elems * 4);
  return dI && dO && hip_ok(hipMemcpy(dI, in, in_elems * 4, hipMemcpyHostToDevice), "H2D") && hip_ok(fn(dI, dO), "launch") &&
         hip_ok(hipMemcpy(out, dO, out_elems * 4, hipMemcpyDeviceToHost), "D2H");
}

void bestla_layernormalization(int norm_count, int norm_size, bool isrms, float epsilon, const float* FpIn,
                               float* FpOut) {
  ns::HostScope host_scope("bestla_layernormalization");
  std::lock_guard<std::mutex> host_lock(g_host_mu);
  CachePin pin;
  const size_t n = size_t(norm_count) * norm_size;
  if (!have_device() || !host_unary(n, n, FpIn, FpOut, [&](const float* i, float* o) {
        return launch_rmsnorm(norm_count, norm_size, isrms, epsilon, i, o, nullptr);
      }))
    invalid_parameters("bestla_layernormalization");
}

static void host_binary(const char* who, int batch, int vsize, const float* tensor, const float* vector, int vstep,
                        float* out, bool mul) {
  std::lock_guard<std::mutex> host_lock(g_host_mu);
  CachePin pin;
  if (batch <= 0 || vsize <= 0) return;  // nothing to do (and batch - 1 below must not wrap)
  bool ok = have_device();
  if (ok) {
    const size_t n = size_t(batch) * vsize;
    const size_t vn = size_t(batch - 1) * vstep + vsize;
    if (zero_copy_enabled() && (2 * n + vn) * 4 <= kZeroCopyMaxBytes) {  // decode-sized: see host_unary
      float *hT = nullptr, *hV = nullptr, *hO = nullptr;
      float* zT = mapped(g_ha, n * 4, &hT);
      float* zV = mapped(g_hd, vn * 4, &hV);
      float* zO = mapped(g_hc, n * 4, &hO);
      if (zT && zV && zO) {
        memcpy(hT, tensor, n * 4);
        memcpy(hV, vector, vn * 4);
        ok = hip_ok(launch_bcast_binary(batch, vsize, zT, zV, vstep, zO, mul, nullptr), "launch") &&
             hip_ok(hipStreamSynchronize(nullptr), "synchronize");
        if (ok) memcpy(out, hO, n * 4);
        if (!ok) invalid_parameters(who);
        return;
      }
      (void)hipGetLastError();
    }
    float* dT = (float*)g_sa.get(n * 4);
    float* dV = (float*)g_sd.get(vn * 4);
    float* dO = (float*)g_sc.get(n * 4);
    ok = dT && dV && dO && hip_ok(hipMemcpy(dT, tensor, n * 4, hipMemcpyHostToDevice), "H2D") &&
         hip_ok(hipMemcpy(dV, vector, vn * 4, hipMemcpyHostToDevice), "H2D") &&
         hip_ok(launch_bcast_binary(batch, vsize, dT, dV, vstep, dO, mul, nullptr), "launch") &&
         hip_ok(hipMemcpy(out, dO, n * 4, hipMemcpyDeviceToHost), "D2H");
  }
  if (!ok) invalid_parameters(who);
}
void bestla_mul(int batch, int vsize, const float* tensor, const float* vector, int vstep, float* out) {
  ns::HostScope host_scope("bestla_mul");
  host_binary("bestla_mul", batch, vsize, tensor, vector, vstep, out, true);
}
void bestla_add(int batch, int vsize, const float* tensor, const float* vector, int vstep, float* out) {
  ns::HostScope host_scope("bestla_add");
  host_binary("bestla_add", batch, vsize, tensor, vector, vstep, out, false);
}

}  // extern "C"
