// ns_api.cpp — C ABI of libns_hip.so (declared in include/ns_bestla.h).
//
// Mirrors the reference's operator boundary:
//   neural_speed/core/ne_bestla.h:21-83                      (extern "C" surface, part 1)
//   neural_speed/core/layers/inner_product.cpp:20-36         (bestla_f32f32_{get_workspace_size,forward})
//   neural_speed/core/layers/bestla_gemm.cpp:508-749         (BTLAGemmBatchDriver / PackBSize / QuantPackB / PackB / UnPackB)
//   neural_speed/core/layers/ip_fusion_qkv.cpp:155-307, ip_fusion_ffn.cpp:20-29,724-779
//   neural_speed/core/layers/ne_bestla.cpp:19-164
// Unlike the reference, which re-parses the blob header (heap alloc + delete) on every call
// (bestla_gemm.cpp:514/:617), a blob pointer is parsed once: the first forward that sees it re-lays the weight out
// for MI355X in HBM and caches blob pointer -> device weight.  There is no CPU compute fallback anywhere in this
// file: without a HIP device every compute entry reports an error.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ns_bestla.h"
#include "ns_common.h"
#include "ns_route.h"

using namespace ns;  // NOLINT

namespace {

std::mutex g_mu;
// The host-pointer entry points share process-wide staging buffers (and the default stream).  The reference runs them
// from one thread at a time (n_tasks = 1, ne_bestla.cpp:270-272); callers that do not are serialised here.
std::mutex g_host_mu;
// Per calling thread, like errno: a failure on one thread is never reported to (or overwritten by) another.
thread_local std::string g_err;
int g_pack_core = NS_CORE_AUTO;
struct CacheEntry {
  ns_weight* w;
  uint64_t fingerprint;
  uint64_t last_use;  // g_cache_tick at the last hit: the eviction order when NS_CACHE_MAX_BYTES caps the cache
};
std::unordered_map<const void*, CacheEntry> g_cache;  // host blob pointer -> device weight (part-1 API)
uint64_t g_cache_tick = 0;
// Pinning against the NS_CACHE_MAX_BYTES eviction: every host entry that looks weights up opens a CachePin for its
// duration.  While any pin is open, entries touched since the OLDEST open pin began (last_use > g_pin_floor) are in
// use by some call — a fused entry holds up to three of them at once — and are never evicted; if that leaves the
// cache over its cap the cap is exceeded until the calls return (q was freed while k / v were loaded).
int g_pin_count = 0;
uint64_t g_pin_floor = 0;
struct CachePin {
  CachePin() {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_pin_count++ == 0) g_pin_floor = g_cache_tick;
  }
  ~CachePin() {
    std::lock_guard<std::mutex> lk(g_mu);
    --g_pin_count;
  }
  CachePin(const CachePin&) = delete;
  CachePin& operator=(const CachePin&) = delete;
};
size_t g_cache_bytes = 0;

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

bool hip_ok(hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return false;
}

bool have_device() {
  static int count = -1;
  if (count < 0) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    count = c;
  }
  if (count <= 0) set_error("no HIP device visible: libns_hip.so has no CPU fallback");
  // every entry point passes here first: drop a stale runtime error (another library's failed call, an invalidated
  // stream capture ...) so that the hipGetLastError() after our own launches reports only those launches
  if (count > 0) (void)hipGetLastError();
  return count > 0;
}

// f4 value tables (reference: bestla/bestla/bestla_utils.h:749-789), rounded to fp16 for the MFMA operand
const float kNF4[16] = {0.f,
                        -0.6961928009986877f,
                        -0.5250730514526367f,
                        -0.39491748809814453f,
                        -0.28444138169288635f,
                        -0.18477343022823334f,
                        -0.09105003625154495f,
                        -1.f,
                        0.07958029955625534f,
                        0.16093020141124725f,
                        0.24611230194568634f,
                        0.33791524171829224f,
                        0.44070982933044434f,
                        0.5626170039176941f,
                        0.7229568362236023f,
                        1.0f};
const float kBNB[8] = {0.f, 5.208333333e-03f, 0.66666667f, 1.f, 0.33333333f, 0.5f, 0.16666667f, 0.25f};
const float kE2M1[8] = {0.f, 0.010416666666666666f, 0.16666666666666666f, 0.25f, 0.3333333333333333f,
                        0.5f, 0.6666666666666666f, 1.f};

// sizes and strides of the device arrays from (ntiles, ksteps, srows, sps, scale dtype, asym)
void set_strides(ns_weight* w, int force_interleave = -1) {
  const uint32_t sbytes = dt_bits(w->scale_dt) / 8;
  const uint32_t cb = 16u * w->sps * sbytes, zb = w->asym ? 16u * w->sps : 0u;
  static const bool no_il = getenv("NS_NO_INTERLEAVE") != nullptr;  // diagnostics
  w->interleaved = force_interleave >= 0 ? force_interleave != 0 : (w->srows == w->ksteps) && !no_il;
  const uint32_t rec = w->code_rec;  // 1024, or the bit planes' own bytes in a native clone
  if (w->interleaved) {
    w->qstride = w->sstride = w->zstride = rec + cb + zb;
    w->codes_bytes = size_t(w->ntiles) * w->ksteps * w->qstride;
    w->scales_bytes = w->codes_bytes - rec;
    w->zps_bytes = w->asym ? w->codes_bytes - rec - cb : 0;
  } else {
    w->qstride = rec;
    w->sstride = cb;
    w->zstride = 16u * w->sps;
    w->codes_bytes = size_t(w->ntiles) * w->ksteps * rec;
    w->scales_bytes = size_t(w->ntiles) * w->srows * cb;
    w->zps_bytes = w->asym ? size_t(w->ntiles) * w->srows * 16 * w->sps : 0;
  }
}

// Decide the device layout for a parsed blob; returns false (with error) for formats the kernels do not cover.
bool plan_weight(const BlobView& v, ns_weight* w) {
  w->n = v.n;
  w->k = v.k;
  w->qtype = v.dtype;
  w->blocksize = v.blocksize;
  w->scale_dt = v.scale_dt;
  w->asym = v.asym();
  if (v.prologue == 1 && dt_is_int(v.dtype) && dt_bits(v.dtype) >= 1 && dt_bits(v.dtype) <= 4) {
    w->kind = WK_INT4;  // S1..S3 are widened to nibbles by the repack (HBM holds 4 bits per weight for them)
  } else if (v.prologue == 1 && dt_is_int(v.dtype) && dt_bits(v.dtype) >= 5 && dt_bits(v.dtype) <= 8) {
    w->kind = WK_INT8;  // S5..S7 widened to bytes
  } else if (v.prologue == 2 && dt_is_f4(v.dtype)) {
    w->kind = WK_F4;
    for (int i = 0; i < 16; i++) {
      float f = v.dtype == DT_F4_NF4 ? kNF4[i] : ((v.dtype == DT_F4_BNB ? kBNB[i & 7] : kE2M1[i & 7]) * ((i & 8) ? -1.f : 1.f));
      w->lut[i] = (_Float16)f;
      w->lutf[i] = f;
    }
  } else if (v.prologue == 2 && dt_is_f8(v.dtype)) {
    w->kind = WK_F8;
    if (v.scale_dt == DT_F8_E8M0) w->scale_dt = DT_F32;  // shared exponents are expanded to fp32 scales by the repack
  } else {
    set_error("weight dtype not supported by the MI355X kernels yet (supported: S1..S8, F4_NF4, F4_BNB, F4_E2M1, F8_E4M3, F8_E5M2)");
    return false;
  }
  if (v.shuf_bytes && v.shuf_bytes != uint64_t(v.k) * sizeof(int)) {
    set_error("blob: shuffle-index section does not hold K entries");
    return false;
  }
  if (v.scale_dt != DT_F32 && v.scale_dt != DT_BF16 && v.scale_dt != DT_F16 &&
      !(v.scale_dt == DT_F8_E8M0 && w->kind == WK_F8)) {
    set_error("scale dtype not supported (F32/BF16/F16; F8_E8M0 with fp8 weights)");
    return false;
  }
  w->kstep_len = (w->kind == WK_INT8 || w->kind == WK_F8) ? 64 : 128;
  w->ntiles = (v.n + 15) / 16;
  w->ksteps = (v.k + w->kstep_len - 1) / w->kstep_len;
  const int bs = v.blocksize;
  if (bs >= v.k) {  // per-channel (the reference stores blocksize = KPad): one scale row
    w->sps = 1;
    w->srows = 1;
  } else if (bs < w->kstep_len) {
    if (bs % 32 != 0 || w->kstep_len % bs != 0) {
      set_error("group size must be a multiple of 32 (and divide 128) for the MI355X kernels");
      return false;
    }
    w->sps = w->kstep_len / bs;
    w->srows = w->ksteps;
  } else if (bs == w->kstep_len) {
    w->sps = 1;
    w->srows = w->ksteps;
  } else if (bs % w->kstep_len == 0) {
    w->sps = 1;
    w->srows = (v.k + bs - 1) / bs;
  } else {
    set_error("group size must be a multiple of 128 when larger than 128");
    return false;
  }
  const int sbytes = dt_bits(v.scale_dt) / 8;
  set_strides(w);
  // reference benchmark formula (ut/bestla_benchmark.cpp:583-586): packed codes + scales (+ zero points)
  const uint64_t nblk = (uint64_t(v.k) + bs - 1) / bs;
  w->stream_bytes = uint64_t(v.n) * v.k * dt_bits(v.dtype) / 8 + uint64_t(v.n) * nblk * sbytes +
                    (w->asym ? uint64_t(v.n) * nblk : 0);
  return true;
}

bool alloc_weight(ns_weight* w, void* ext = nullptr, size_t ext_bytes = 0) {
  // ONE allocation per weight: [codes | scales | zero points], each 256-byte aligned, so that a kernel addresses all
  // streams from one base with 32-bit offsets (s_off / z_off)
  auto pad = [](size_t b) { return (b + 255) & ~size_t(255); };
  size_t s_off, z_off, total;
  if (w->interleaved) {  // scales / zps live inside the record stream
    const size_t cb = size_t(16) * w->sps * (dt_bits(w->scale_dt) / 8);
    s_off = w->code_rec;
    z_off = w->asym ? w->code_rec + cb : 0;
    total = pad(w->codes_bytes);
  } else {
    s_off = pad(w->codes_bytes);
    z_off = w->asym ? s_off + pad(w->scales_bytes) : 0;
    total = s_off + pad(w->scales_bytes) + pad(w->zps_bytes);
  }
  uint8_t* base = nullptr;
  if (ext && total <= ext_bytes && (reinterpret_cast<uintptr_t>(ext) & 255) == 0) {
    base = static_cast<uint8_t*>(ext);  // the caller's slice holds the streaming layout: no allocation of its own
    w->external = true;
  } else if (!hip_ok(hipMalloc((void**)&base, total), "hipMalloc(weight)")) {
    return false;
  }
  w->codes = reinterpret_cast<uint4*>(base);  // owned by `w` from here on: ns_hip_weight_free releases it on any later failure
  w->scales = base + s_off;
  w->zps = w->asym ? reinterpret_cast<int8_t*>(base + z_off) : nullptr;
  w->s_off = total < (size_t(1) << 32) ? uint32_t(s_off) : 0;
  w->z_off = total < (size_t(1) << 32) ? uint32_t(z_off) : 0;
  w->single_span = total < (size_t(1) << 32);
  w->alloc_bytes = total;
  hipGetDevice(&w->device);
  return true;
}

// bytes of one k-step's bit planes for the 16 columns of a tile (the decode kernel's native records): nibble-order formats span
// 128 k (2-bit plane 512 B, 1-bit plane 256 B), byte-order formats 64 k (4-bit plane 512 B + one more plane of 256 B)
uint32_t plane_record_bytes(int bits) {
  switch (bits) {
    case 1: return 256;
    case 2: return 512;
    case 3: return 768;
    case 5: return 768;
    case 6: return 768;
    default: return 0;  // 4, 8: the container is the format; 7: no shorter form (ns_kernels.hip repack_planes_kernel)
  }
}
// S1..S3 / S5..S7: build the native clone (ns_common.h ns_weight::native) from the same reference sections, on the same stream.
// Failure to allocate is not an error: the weight then streams its widened records at decode too.
// Off by default (ns_hip_set_tuning("planes_load", 1) / NS_PLANES=1 before the weights are loaded): measured on this chip the
// decode kernel is bound by its per-record and per-launch costs, not by bytes — native records run 0.89-0.98 x (1-3 bit) and
// 1.00-1.07 x (5, 6 bit) the widened ones on the 7B FFN shapes (profiles/r04aq_planes_native_vs_widened.txt) — and the clone
// is a second copy of the weight in HBM.
static std::atomic<int> g_planes_load{-1};
void set_planes_load(int on) { g_planes_load.store(on != 0); }
void add_native_planes(const RepackArgs& ra, ns_weight* w, hipStream_t st) {
  int on = g_planes_load.load();
  if (on < 0) {
    const char* e = getenv("NS_PLANES");
    on = e ? atoi(e) != 0 : 0;
    g_planes_load.store(on);
  }
  const int bits = dt_bits(w->qtype);
  if (!on || (w->kind != WK_INT4 && w->kind != WK_INT8) || !plane_record_bytes(bits) || w->native) return;
  ns_weight* c = new ns_weight(*w);
  c->native = nullptr, c->shuf = nullptr, c->external = false, c->load_pending = false;
  c->codes = nullptr, c->scales = nullptr, c->zps = nullptr;
  c->pl_bits = uint8_t(bits);
  c->code_rec = plane_record_bytes(bits);
  set_strides(c, w->interleaved ? 1 : 0);
  RepackArgs rc = ra;
  rc.flags = nullptr;
  if (!alloc_weight(c) || launch_repack(rc, c, st) != hipSuccess) {
    (void)hipGetLastError();
    ns_hip_reset_error();
    ns_hip_weight_free(c);
    return;
  }
  w->native = c;
}

template <typename T>
struct DevBuf {
  T* p = nullptr;
  ~DevBuf() {
    if (p) hipFree(p);
  }
  bool alloc(size_t count) { return hip_ok(hipMalloc((void**)&p, count * sizeof(T) + 16), "hipMalloc(temp)"); }
};

// gemm2 multiplies fp16 weights that already carry their group scale: pick the power of two that brings the largest
// |scale| to [2^5, 2^6).  |code - zp| <= 383, so scaled weights stay below 2^15 (no overflow however large the
// original weights are), and only groups more than 2^-19 below the largest one drop under fp16's normal range — bits
// far beneath the 1e-3 budget relative to the output.  Powers of two change no rounding inside the normal range.
// fp8 weights: the fp16 operand is code value * scale, and a code value is up to 480 (E4M3: 2^-7 .. 1.875 * 2^8) or 57344 (E5M2:
// 2^-15 .. 1.75 * 2^15; exponent field 31 is refused at load) — the largest |scale| goes to [2^6, 2^7) (480 * 2^7 = 61440) or to
// [2^-1, 1), both below fp16's 65504.  `low_scales` (launch_scale_spread with gemm_f8_scale_drop below): some group's scale would
// leave fp16's normal range under that factor — the weight then stays on the first-generation GEMM (ns_weight::g2_ok).
int gemm_f8_scale_top(uint32_t qtype) { return qtype == DT_F8_E5M2 ? 0 : 7; }
// fp32 scales: every scale * g2_pre stays a NORMAL fp16 number (>= 2^-14: the product code * scale is then rounded once, 2^-12
// relative, like the integer formats').  E8M0 scales are powers of two, exact as fp16 subnormals as well: down to 2^-20, where a
// group's largest code (>= 2^8) still lies 12 bits above fp16's subnormal step of 2^-24.
int gemm_f8_scale_drop(uint32_t qtype, uint32_t src_scale_dt) { return gemm_f8_scale_top(qtype) + (src_scale_dt == DT_F8_E8M0 ? 20 : 14); }
void set_gemm_scale_range(ns_weight* w, uint32_t smax_bits, bool low_scales = false) {
  w->g2_pre = w->g2_post = 1.f;
  w->g2_ok = !(w->kind == WK_F8 && low_scales);
  float smax;
  memcpy(&smax, &smax_bits, 4);
  if (!(smax > 0.f)) return;
  int e;
  frexpf(smax, &e);           // smax = f * 2^e, f in [0.5, 1)
  int shift = (w->kind == WK_F8 ? gemm_f8_scale_top(w->qtype) : 6) - e;  // smax * 2^shift in [2^5, 2^6) (fp8: see above)
  if (shift > 100 || shift < -100) w->g2_ok = w->kind != WK_F8;  // (fp8 has no headroom for a clamped factor)
  if (shift > 100) shift = 100;
  if (shift < -100) shift = -100;
  w->g2_pre = ldexpf(1.f, shift);
  w->g2_post = ldexpf(1.f, -shift);
}

// every shuffle index must address a column of A
bool check_shuffle(const ns_weight* w) {
  std::vector<int> h(size_t(w->k));
  if (!hip_ok(hipMemcpy(h.data(), w->shuf, h.size() * sizeof(int), hipMemcpyDeviceToHost), "D2H shuffle")) return false;
  for (int v : h)
    if (v < 0 || v >= w->k) {
      set_error("blob: shuffle index outside [0, K)");
      return false;
    }
  return true;
}

// ---- DQ8_BNB scales (round 4) ---------------------------------------------------------------------------------------------
// The reference can store a weight's scales double-quantised (StorageWeightKBlockN*::mDqBlockSize != 0, bestla_storage.h:750-759): one
// u8 code per scale into the bitsandbytes dynamic map + an fp32 maximum per block of `dq_blocksize` scales + one fp32 offset.  At load
// they are expanded to the fp32 scales its kernels dequantise with (dq8_get_fp_scale, kernel_ref.h:1980-1992); everything behind the
// load sees an fp32-scale weight.  Readable for the two weight types the reference itself reads them for: S4 and NF4.
// The map: create_dynamic_map(signed, 7 exponent bits, 8 bits) of bitsandbytes, written with five decimals (bestla_utils.h:791-...).
const float* dq8_lut_device() {
  static float* d = nullptr;
  static std::once_flag once;
  std::call_once(once, [] {
    std::vector<double> data;
    for (int i = 0; i < 7; i++) {
      const int items = 1 << i;
      const double mag = std::pow(10.0, -6 + i);
      for (int j = 0; j < items; j++) {
        const double b0 = 0.1 + 0.9 * double(j) / double(items), b1 = 0.1 + 0.9 * double(j + 1) / double(items);
        data.push_back(mag * (b0 + b1) / 2.0);
        data.push_back(-mag * (b0 + b1) / 2.0);
      }
    }
    data.push_back(0.0);
    data.push_back(1.0);
    std::sort(data.begin(), data.end());
    float lut[256];
    for (int i = 0; i < 256; i++) {
      char buf[32];
      snprintf(buf, sizeof(buf), "%.5f", data[size_t(i)]);
      lut[i] = strtof(buf, nullptr);
    }
    if (hipMalloc((void**)&d, sizeof(lut)) != hipSuccess || hipMemcpy(d, lut, sizeof(lut), hipMemcpyHostToDevice) != hipSuccess) d = nullptr;
  });
  return d;
}
// `out` (device, csize floats) <- the expanded scales; v2 = the view the rest of the load works with
bool dq8_expand(const BlobView& v, const uint8_t* d_codes, const float* d_dq, float* out, BlobView* v2, hipStream_t st) {
  const bool s4 = v.prologue == 1 && dt_is_int(v.dtype) && dt_bits(v.dtype) == 4, nf4 = v.prologue == 2 && v.dtype == DT_F4_NF4;
  if (!s4 && !nf4) {
    set_error("blob: DQ8_BNB scales are read for S4 and NF4 weights only (as in the reference: bestla_prologue_b.h:742-751, :1298-1306)");
    return false;
  }
  const float* lut = dq8_lut_device();
  if (!lut || !d_dq) {
    set_error("DQ8_BNB scales: no code map / no double-quantisation section on the device");
    return false;
  }
  const int rows = int(v.csize / uint64_t(v.cstep));
  if (!hip_ok(launch_dq8_expand(d_codes, d_dq, lut, out, rows, v.cstep, v.n, v.dq_blocksize, uint32_t(v.dq_bytes / 4 - 1), st), "dq8 expand"))
    return false;
  *v2 = v;
  v2->scale_dt = DT_F32;
  v2->s_bytes = v.csize * 4;
  v2->dq_bytes = 0, v2->dq_off = 0;
  return true;
}

// sections already in device memory -> device weight
ns_weight* weight_from_device_sections(const BlobView& v_in, const uint8_t* dq, const uint8_t* ds, const int8_t* dz,
                                       hipStream_t st, const float* d_dqsec = nullptr) {
  BlobView v = v_in;
  DevBuf<float> dq8_scales;  // lives until the synchronisation at the end of this function
  if (v_in.scale_dt == DT_DQ8_BNB) {
    if (!dq8_scales.alloc(size_t(v_in.csize)) || !dq8_expand(v_in, ds, d_dqsec, dq8_scales.p, &v, st)) return nullptr;
    ds = reinterpret_cast<const uint8_t*>(dq8_scales.p);
  }
  ns_weight* w = new ns_weight();
  if (!plan_weight(v, w) || !alloc_weight(w)) {
    ns_hip_weight_free(w);
    return nullptr;
  }
  RepackArgs ra{dq, ds, dz, v.ntile(), v.packrow(), v.kpad, v.npad, v.cstep, int((v.kpad + v.blocksize - 1) / v.blocksize)};
  ra.src_scale_dt = v.scale_dt;
  DevBuf<uint32_t> dinfo;  // [0] largest |scale| (fp32 bits), [1] out-of-range code flag
  uint32_t info[2] = {0, 0};
  bool ok = dinfo.alloc(2) && hip_ok(hipMemsetAsync(dinfo.p, 0, 8, st), "memset");
  if (ok) {
    ra.flags = dinfo.p + 1;
    ok = hip_ok(launch_repack(ra, w, st), "repack") && (add_native_planes(ra, w, st), true) &&
         hip_ok(launch_scale_absmax(ds, v.s_bytes / (dt_bits(v.scale_dt) / 8), v.scale_dt, dinfo.p, st, v.cstep, int(v.n)), "scale range") &&
         (w->kind != WK_F8 || hip_ok(launch_scale_spread(ds, v.s_bytes / (dt_bits(v.scale_dt) / 8), v.scale_dt, gemm_f8_scale_drop(w->qtype, v.scale_dt), dinfo.p, st, v.cstep, int(v.n)), "scale spread")) &&
         hip_ok(hipMemcpyAsync(info, dinfo.p, 8, hipMemcpyDeviceToHost, st), "load info D2H") &&
         hip_ok(hipStreamSynchronize(st), "sync after repack");
  }
  if (ok && (info[1] & 1)) {
    set_error("F8_E5M2 blob holds codes with exponent field 31 (beyond the reference quantizer's max_norm and fp16)");
    ok = false;
  }
  if (!ok) {
    ns_hip_weight_free(w);
    return nullptr;
  }
  set_gemm_scale_range(w, info[0], (info[1] & 2) != 0);
  return w;
}

// The reference treats a blob as immutable for the model's lifetime (it points into the model mmap,
// model_files.h:1564-1571), so the pointer is the cache key.  To stay safe when a caller recycles the address for a
// different weight, each hit is validated against a cheap content fingerprint (header + 256 sampled words).
uint64_t blob_fingerprint(const void* blob) {
  const uint8_t* b = static_cast<const uint8_t*>(blob);
  uint64_t size;
  memcpy(&size, b, 8);
  if (size < 64 || size > (uint64_t(1) << 40)) return 0;
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](uint64_t v) {
    h ^= v;
    h *= 1099511628211ull;
  };
  for (int i = 0; i < 6; i++) {
    uint64_t v;
    memcpy(&v, b + 8 * i, 8);
    mix(v);
  }
  const uint64_t words = size / 8;
  const uint64_t stride = words / 256 ? words / 256 : 1;
  for (uint64_t wd = 8; wd < words; wd += stride) {
    uint64_t v;
    memcpy(&v, b + 8 * wd, 8);
    mix(v ^ wd);
  }
  return h ? h : 1;
}

ns_weight* cached_weight(const void* blob) {
  if (!blob) {
    set_error("blob: null pointer");
    return nullptr;
  }
  const uint64_t fp = blob_fingerprint(blob);
  // one lock over lookup + upload + insert: two threads presenting the same new blob must not both upload it
  // (the loser's device copy would leak and its pointer dangle after the next cache_clear)
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_cache.find(blob);
  if (it != g_cache.end()) {
    if (it->second.fingerprint == fp) {
      it->second.last_use = ++g_cache_tick;
      return it->second.w;
    }
    g_cache_bytes -= std::min(g_cache_bytes, it->second.w->alloc_bytes);
    ns_hip_weight_free(it->second.w);  // the address now holds a different blob
    g_cache.erase(it);
  }
  ns_weight* w = ns_hip_weight_from_blob(blob, nullptr);
  if (!w) return nullptr;
  // optional cap (NS_CACHE_MAX_BYTES, default unlimited: a model's weights are a fixed set): least recently used
  // device copies go first — except the ones a call in flight may hold (CachePin above).
  static const size_t cap = getenv("NS_CACHE_MAX_BYTES") ? strtoull(getenv("NS_CACHE_MAX_BYTES"), nullptr, 10) : 0;
  g_cache_bytes += w->alloc_bytes;
  while (cap && g_cache_bytes > cap && !g_cache.empty()) {
    auto victim = g_cache.end();
    for (auto jt = g_cache.begin(); jt != g_cache.end(); ++jt) {
      if (g_pin_count > 0 && jt->second.last_use > g_pin_floor) continue;  // in use by a call in flight
      if (victim == g_cache.end() || jt->second.last_use < victim->second.last_use) victim = jt;
    }
    if (victim == g_cache.end()) break;  // the working set of the calls in flight exceeds the cap: keep it
    g_cache_bytes -= std::min(g_cache_bytes, victim->second.w->alloc_bytes);
    ns_hip_weight_free(victim->second.w);
    g_cache.erase(victim);
  }
  g_cache[blob] = CacheEntry{w, fp, ++g_cache_tick};
  return w;
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

// numerics mode (ns_hip_set_compute_mode / NS_COMPUTE): 0 = fp16 activations x dequantised weights, fp32 accumulate
// (default); 1 = the reference's int8-compute semantics for integer weights (ns_i8ref.hip)
int env_compute_mode() {
  const char* e = getenv("NS_COMPUTE");
  return e && (!strcmp(e, "ref_int8") || !strcmp(e, "1")) ? NS_COMPUTE_REF_INT8 : NS_COMPUTE_FP16;
}
std::atomic<int> g_compute_mode{env_compute_mode()};
bool ref_int8_for(const ns_weight* w) { return g_compute_mode.load() == NS_COMPUTE_REF_INT8 && w && i8ref_supported(w); }

// rows up to which the weight-streaming kernel is used; above, the tiled MFMA GEMM (measured crossover)
constexpr int kSmallMMax = 64;
// a carried RMS norm (ns_norm_link) is honoured by gemv_kernel only: refuse everything that would leave its envelope
bool link_ok(const ns_norm_link* link, const ns_weight* w, int m, const void* dA16) {
  if (m > 16 || !dA16 || w->shuf || ref_int8_for(w)) {
    set_error("norm link: needs m <= 16, the fp16 shadow of A, no activation shuffle and the fp16 compute mode");
    return false;
  }
  if (link->in_ssq && (link->in_parts < 1 || link->norm_size < 1 || link->in_stride < link->in_parts || (link->in_stride & 3) ||
                       (reinterpret_cast<uintptr_t>(link->in_ssq) & 15))) {
    set_error("norm link: in_ssq must be 16-byte aligned with in_stride >= in_parts, a multiple of 4");
    return false;
  }
  return true;
}

// rows from which the TILED kernel serves a weight of this shape although most of its tile is padding (measurements: forward_impl)
int tiled_from_rows(const ns_weight* w) {
  return w->ntiles >= 512 ? 17 : w->ntiles >= 256 ? (w->k >= 8192 ? 17 : 33) : 1 << 30;
}

// int8-reference decode launch: the kernel quantizes the activations itself where it can; where it cannot it says so, the quantizer
// launch runs, and the launch is repeated on the codes
hipError_t launch_gemv_i8(const SmallMArgs& a, I8Act* q, hipStream_t st) {
  hipError_t e = launch_gemv(a, st);
  if (e == hipErrorNotReady) {
    e = i8_quantize_finish(q, st);
    if (e == hipSuccess) e = launch_gemv(a, st);
  }
  return e;
}

int forward_impl(const float* dA, const ns_weight* w, float* dC, int m, int lda, int ldc, int epilogue,
                 const float* dD, int ldd, hipStream_t st, const void* dA16 = nullptr, void* dC16 = nullptr,
                 bool reuse_aq = false, const ns_norm_link* link = nullptr) {
  if (!w || (!dA && !dA16) || (!dC && !dC16) || m <= 0) {
    set_error("forward: null argument");
    return -1;
  }
  if (w->load_failed) {
    set_error("forward: this weight's load was rejected (ns_hip_weight_finish_load)");
    return -1;
  }
  if (!dA || !dC) {
    // fp16-only activations (the producer wrote its shadow only) and / or an fp16-only output (the consumer is this library's next
    // GEMM): the tiled kernel multiplies fp16 activations as they are and can leave the fp32 store out (round 5)
    if (w->shuf || ref_int8_for(w) || link || !gemm3_takes(w)) {
      set_error("forward: fp16-only activations / outputs need a weight the tiled kernel takes as is (no act-order shuffle, no int8-reference mode; fp8 with the g3_f8 switch on and group scales within its range rule)");
      return -1;
    }
    SmallMArgs a{};
    a.a = dA, a.a16 = dA16, a.lda = lda, a.m = m, a.ldc = ldc, a.nseg = 1;
    a.seg[0] = {w, dC, dC16};
    a.epilogue = epilogue, a.d = dD, a.ldd = ldd;
    const hipError_t e = launch_gemm2(a, st);
    if (e == hipErrorNotSupported) {
      set_error("forward: fp16-only activations / outputs are outside the tiled kernel's envelope (K a multiple of 64, lda a multiple of 8, 16-byte aligned)");
      return -1;
    }
    return hip_ok(e, "gemm launch (fp16-only operand)") ? 0 : -1;
  }
  if (link && !link_ok(link, w, m, dA16)) return -1;
  if (!smallm_supported(w, m)) {
    set_error("forward: weight format not supported");
    return -1;
  }
  if (w->shuf) {  // GPTQ act-order blob: gather A'[j] = A[shuf[j]] into scratch first (prologue_a.h:322-330)
    float* ga = static_cast<float*>(stream_scratch(st, size_t(m) * w->k * 4, 3));
    if (!ga) {
      set_error("forward: no scratch for the activation shuffle (out of device memory)");
      return -1;
    }
    if (!hip_ok(launch_gather_cols(dA, lda, w->shuf, ga, m, w->k, st), "activation shuffle")) return -1;
    dA = ga;
    lda = w->k;
    dA16 = nullptr;  // the caller's fp16 shadow is in the unshuffled order
  }
  if (ref_int8_for(w) && m <= 4) {  // decode-sized: the streaming kernel's int8-reference variant (gemv_kernel XV = 3)
    I8Act q;
    if (hip_ok(i8_quantize_for_decode(dA, lda, w, m, st, reuse_aq && !w->shuf, &q), "activation quantization")) {
      SmallMArgs a{};
      a.a = dA, a.lda = lda, a.m = m, a.ldc = ldc, a.nseg = 1;
      a.seg[0] = {w, dC, dC16};
      a.epilogue = epilogue, a.d = dD, a.ldd = ldd;
      a.i8 = &q;
      const hipError_t e = launch_gemv_i8(a, &q, st);
      if (e == hipSuccess) return 0;
      if (e != hipErrorNotSupported) return hip_ok(e, "int8-reference decode launch") ? 0 : -1;
      reuse_aq = false;  // outside that kernel's envelope: the general int8-reference kernel, with its own scratch
    } else {
      return -1;
    }
  }
  if (ref_int8_for(w))  // opt-in: quantize A to u8 per k-block and accumulate integer dots, like the CPU int8 cores
    return hip_ok(launch_i8ref(dA, lda, w, dC, dC16, m, ldc, epilogue, dD, ldd, st, reuse_aq && !w->shuf),
                  "int8-reference forward") ? 0 : -1;
  // M <= 64: weight-streaming kernel (HBM-bound); larger M: tiled MFMA GEMM (weights reused across 128 rows)
  SmallMArgs a{};
  a.a = dA;
  a.a16 = dA16;
  a.lda = lda;
  a.m = m;
  a.ldc = ldc;
  a.nseg = 1;
  a.seg[0] = {w, dC, dC16};
  a.epilogue = epilogue;
  a.d = dD;
  a.ldd = ldd;
  a.dual = false;
  a.c2 = nullptr;
  a.link = link;
  static const int small_max = getenv("NS_SMALLM_MAX") ? atoi(getenv("NS_SMALLM_MAX")) : kSmallMMax;  // diagnostics
  // Up to 16 rows the streaming kernel always wins.  From 17 to 64 rows every 16-column workgroup of it stages all rows
  // of A over the whole K from L2, ntiles x m x K x sizeof(A element) bytes in total at about 6 TB/s: measured against
  // the tiled GEMM (scripts/m_small_sweep.py) the break-even is near 140 MB of such staging traffic — 4096 x 4096 stays
  // on the streaming kernel up to 64 rows with an fp16 shadow (21 vs 25 us), 14336 x 4096 leaves it at 17 (53 vs 44 us
  // at 32 rows), fp32 activations leave earlier.
  double staging = double(w->ntiles) * m * w->k * (dA16 ? 2.0 : 4.0);
  // Where the TILED kernel (64-row tile up to 64 rows) beats the streaming one although most of its tile is padding — every
  // 16-column workgroup of the streaming kernel stages all rows of A, the tiled kernel's 128-column workgroups share them
  // (round 3, scripts/m_sweep.py, profiles/r03_m_sweep.txt; us, streaming -> tiled):
  //   32000 x 4096 (lm_head)   8 rows 39.8 -> 32.1, 16 rows 53.4 -> 32.6   (4 rows: 28.9 vs 32.1, stays)
  //   11008 x 4096             16 rows 17.2 -> 16.7, 17 rows 33.0 -> 17.5, 64 rows 44.8 -> 20.8
  //   4096 x 11008             16 rows 24.1 -> 19.7 (12 rows level),  4096 x 4096: 33 rows 15.8 -> 13.4 (below: level or behind)
  // fp8 weights keep the old rule up to 64 rows (streaming / first-generation kernels) and take the tiled kernel from 65 (launch_gemm2
  // refuses them below, docs/kernels/gemm3.md).  NS_TILED_MIN_M: diagnostics (A-B runs).
  static const int tiled_env = getenv("NS_TILED_MIN_M") ? atoi(getenv("NS_TILED_MIN_M")) : 0;
  // Up to 16 rows every call stays on the streaming kernels all the same: their accumulation is exact in fp32 (3e-5 from the
  // fp64 product of the fp16-rounded activations, tests/test_gpu_fullsize.py), the tiled kernel rounds scaled weights to fp16
  // (2e-4), and a decode step's numerics should not depend on the shape of the matrix.
  const int tiled_from = tiled_env > 0 ? tiled_env : tiled_from_rows(w);
  const bool wide_tiled = m >= tiled_from && (w->kind != WK_F8 || (m > 64 && gemm3_takes(w))) && !getenv("NS_SMALLM_MAX");
  const bool small = !wide_tiled && (m <= 16 || (m <= small_max && (staging <= 140e6 || getenv("NS_SMALLM_MAX") != nullptr)));
  // fp32 activations, several rows, many column tiles: one conversion pass to fp16 (about 2 us) halves what every
  // workgroup of the streaming kernel stages (14336 x 4096 at 16 rows: 39 -> 24 us; at 8 rows: 25 -> 18 us)
  if (small && !dA16 && m >= 6 && staging > 60e6 && lda == w->k && w->k % 8 == 0) {
    void* sc = stream_scratch(st, size_t(m) * w->k * 2, 0);
    if (sc && hip_ok(launch_cvt_a16(dA, sc, m, w->k, lda, w->k, st), "activation fp16 pass")) a.a16 = sc;
  }
  if (!hip_ok(small ? launch_smallm(a, st) : launch_gemm(a, st), "gemm launch")) return -1;
  return 0;
}

}  // namespace

namespace ns {
// the device route's replayed QKV launch (ns_route.cpp XK_QKV_ROPE): one row, carried norm on the input, RoPE + fp16 mirror + fp32 cache cells in the epilogue
int qkv_rope_route_forward(const float* dA, const void* dA16, const ns_weight* wq, const ns_weight* wk, const ns_weight* wv, float* cq, float* ck,
                           float* cv, int lda, const ns_norm_link* link, const ns_qkv_rope* rope, const QkvRopeRoute* rr, hipStream_t st) {
  if (!have_device()) return -1;
  const ns_weight* ws[3] = {wq, wk, wv};
  if (!rr) {  // a window's prompt-sized launch (rows: rope->flags' place is taken by the caller's m in `lda`'s partner below): the tiled GEMM carries the epilogue
    set_error("route qkv+rope: prompt-sized calls go through qkv_rope_route_forward_m");
    return -1;
  }
  if (rope && ((rope->flags & NS_QKV_ROPE_NEOX) || rope->mode != 0)) {
    set_error("route qkv+rope: the replayed route is llama's, RoPE mode 0");
    return -1;
  }
  if (!wq || !wk || !wv || !dA16 || !cq || !ck || !cv || !rope) {
    set_error("route qkv+rope: null argument");
    return -1;
  }
  bool same = !ref_int8_for(wq);
  for (int i = 0; i < 3; i++)
    same &= ws[i]->k == wq->k && ws[i]->kind == wq->kind && ws[i]->blocksize == wq->blocksize && ws[i]->scale_dt == wq->scale_dt &&
            ws[i]->asym == wq->asym && ws[i]->qtype == wq->qtype && !ws[i]->shuf && !ws[i]->load_failed;
  if (!same || !smallm_supported(wq, 1) || (link && (link->out_gamma || link->out_ssq)) || (link && !link_ok(link, wq, 1, dA16))) {
    if (same) set_error("route qkv+rope: the launch cannot carry this norm / these weights");
    else set_error("route qkv+rope: needs three weights of one format in the fp16 compute mode");
    return -1;
  }
  SmallMArgs a{};
  a.a = dA, a.a16 = dA16, a.lda = lda, a.m = 1, a.ldc = wq->n, a.nseg = 3;
  float* cs[3] = {cq, ck, cv};
  for (int i = 0; i < 3; i++) a.seg[i] = {ws[i], cs[i], nullptr};
  a.epilogue = NS_EPI_NONE;
  a.link = link;
  a.rope = rope;
  a.rope_route = rr;
  return hip_ok(launch_smallm(a, st), "route qkv+rope launch") ? 0 : -1;
}
// ... and of a window's prompt-sized evaluation (m > 16): the tiled GEMM's fused-QKV launch rotates q / k from a table of m positions, writes the three fp32
// tensors where the graph has them and k / v as fp16 into the kv mirror (rope->kcache16 / vcache16).  -2: the launch does not take this shape (the caller keeps
// its separate launches)
int qkv_rope_route_forward_m(const float* dA, const void* dA16, const ns_weight* wq, const ns_weight* wk, const ns_weight* wv, float* cq, float* ck, float* cv, int m,
                             int lda, int ldc, const ns_qkv_rope* rope, hipStream_t st) {
  if (!have_device()) return -1;
  const ns_weight* ws[3] = {wq, wk, wv};
  if (!wq || !wk || !wv || !dA || !cq || !ck || !cv || !rope || m <= 16) return -2;
  // (fp8 weights from 65 rows: the separate launches the caller keeps below that are the ones that served such a window before)
  bool one = !ref_int8_for(wq) && (wq->kind != WK_F8 || (m > 64 && gemm3_takes(wq) && gemm3_takes(wk) && gemm3_takes(wv)));
  for (int i = 0; i < 3; i++)
    one &= ws[i]->k == wq->k && ws[i]->kind == wq->kind && ws[i]->blocksize == wq->blocksize && ws[i]->scale_dt == wq->scale_dt && ws[i]->asym == wq->asym &&
           ws[i]->qtype == wq->qtype && !ws[i]->shuf && !ws[i]->load_failed;
  if (!one) return -2;
  SmallMArgs a{};
  a.a = dA, a.a16 = dA16, a.lda = lda, a.m = m, a.ldc = ldc, a.nseg = 3;
  float* cs[3] = {cq, ck, cv};
  for (int i = 0; i < 3; i++) a.seg[i] = {ws[i], cs[i], nullptr};
  a.epilogue = NS_EPI_NONE;
  a.rope = rope;
  const hipError_t e = launch_gemm2(a, st);
  if (e == hipErrorNotSupported) return -2;
  return hip_ok(e, "route qkv+rope GEMM launch") ? 0 : -1;
}
void set_error(const std::string& s) { g_err = s; }
bool route_link_weight_ok(const ns_weight* w) { return w && !w->shuf && !w->load_failed && !ref_int8_for(w) && w->kind != WK_F8 && smallm_supported(w, 1); }
}  // namespace ns

extern "C" {

// ------------------------------------------------------------------------------------------------ part 3
void ns_hip_reset_error(void) {
  // drops a sticky HIP error (e.g. after a stream capture was invalidated) and the library's error string
  for (int i = 0; i < 8 && hipGetLastError() != hipSuccess; i++) {
  }
  set_error("");
}

}  // extern "C"  (reopened below)
namespace ns {
namespace {
struct HostProf {
  std::mutex mu;
  std::map<std::string, std::pair<long long, long long>> acc;  // name -> (calls, ns)
  ~HostProf() {
    if (acc.empty()) return;
    long long total = 0;
    for (auto& kv : acc) total += kv.second.second;
    fprintf(stderr, "NS_HOST_PROFILE: host-tensor entries, %.3f ms in total\n", total * 1e-6);
    for (auto& kv : acc)
      fprintf(stderr, "  %-46s calls %7lld  total %10.3f ms  avg %8.1f us\n", kv.first.c_str(), kv.second.first, kv.second.second * 1e-6,
              kv.second.first ? kv.second.second * 1e-3 / kv.second.first : 0.0);
  }
};
HostProf g_host_prof;
bool host_prof_on() {
  static const bool on = getenv("NS_HOST_PROFILE") != nullptr;
  return on;
}
long long now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace
HostScope::HostScope(const char* n) : name(n), t0(host_prof_on() ? now_ns() : 0) {}
HostScope::~HostScope() {
  if (!t0) return;
  const long long dt = now_ns() - t0;
  std::lock_guard<std::mutex> lk(g_host_prof.mu);
  auto& e = g_host_prof.acc[name];
  e.first++, e.second += dt;
}
}  // namespace ns
extern "C" {

void ns_hip_cache_clear(void) {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& kv : g_cache) ns_hip_weight_free(kv.second.w);
    g_cache.clear();
    g_cache_bytes = 0;
  }
  kv_mirrors_clear();  // ns_attn.hip: device mirrors of library-managed kv caches
}

int ns_hip_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

const char* ns_hip_last_error(void) { return g_err.c_str(); }

int ns_hip_blob_validate(const void* host_blob, size_t avail_bytes) {
  // header-only, no device: the checks every loader entry applies (blob_parse -> check_view), plus the caller's bound
  if (!host_blob) {
    set_error("blob: null pointer");
    return -1;
  }
  BlobView v;
  std::string err;
  if (!blob_parse(host_blob, &v, &err)) {
    set_error(err);
    return -1;
  }
  if (avail_bytes && v.size > avail_bytes) {
    set_error("blob: serialized size " + std::to_string(v.size) + " exceeds the " + std::to_string(avail_bytes) + " bytes available");
    return -1;
  }
  return 0;
}

ns_weight* ns_hip_weight_from_blob(const void* host_blob, void* stream) {
  if (!have_device()) return nullptr;
  hipStream_t st = (hipStream_t)stream;
  BlobView v;
  std::string err;
  if (!blob_parse(host_blob, &v, &err)) {
    set_error(err);
    return nullptr;
  }
  const uint8_t* base = static_cast<const uint8_t*>(host_blob);
  DevBuf<uint8_t> dq, ds;
  DevBuf<int8_t> dz;
  if (!dq.alloc(v.q_bytes) || !ds.alloc(v.s_bytes)) return nullptr;
  if (!hip_ok(hipMemcpyAsync(dq.p, base + v.q_off, v.q_bytes, hipMemcpyHostToDevice, st), "H2D codes")) return nullptr;
  if (!hip_ok(hipMemcpyAsync(ds.p, base + v.s_off, v.s_bytes, hipMemcpyHostToDevice, st), "H2D scales")) return nullptr;
  if (v.asym()) {
    if (!dz.alloc(v.z_bytes)) return nullptr;
    if (!hip_ok(hipMemcpyAsync(dz.p, base + v.z_off, v.z_bytes, hipMemcpyHostToDevice, st), "H2D zps")) return nullptr;
  }
  DevBuf<float> ddq;
  if (v.dq_bytes && (!ddq.alloc(size_t(v.dq_bytes / 4)) ||
                     !hip_ok(hipMemcpyAsync(ddq.p, base + v.dq_off, v.dq_bytes, hipMemcpyHostToDevice, st), "H2D double-quantisation section")))
    return nullptr;
  ns_weight* w = weight_from_device_sections(v, dq.p, ds.p, dz.p, st, ddq.p);
  if (w && v.shuf_bytes &&
      (!hip_ok(hipMalloc((void**)&w->shuf, v.shuf_bytes), "hipMalloc(shuffle)") ||
       !hip_ok(hipMemcpy(w->shuf, base + v.shuf_off, v.shuf_bytes, hipMemcpyHostToDevice), "H2D shuffle") ||
       !check_shuffle(w))) {
    ns_hip_weight_free(w);
    return nullptr;
  }
  return w;
}

// ---- load path of the reference's device loader (model_files.h:1515-1527 -> bestla_device_load_storage) ----
// One grow-only staging buffer on the device takes each blob's sections; the repack writes the streaming layout straight
// into `dst` (the slice the graph reserved for the tensor) when it fits there, into an allocation of its own otherwise;
// nothing is synchronised: the two words the load wants back (largest |scale|, out-of-range flag) go to `pinned_info` by an
// asynchronous copy and are consumed by ns_hip_weight_finish_load once the caller has synchronised the stream — once per
// model, not once per tensor.  The host blob may be freed on return (pageable-memory copies return when the source is consumed).
namespace {
struct Staging {
  uint8_t* p = nullptr;
  size_t bytes = 0;
  uint32_t* info = nullptr;  // device: per-load pair of words, a ring of 4096 pairs
  uint32_t next = 0;
};
Staging g_staging;
constexpr uint32_t kInfoRing = 4096;
}  // namespace

ns_weight* ns_hip_weight_load_async(const void* host_blob, void* dst, uint64_t dst_bytes, void* stream, uint32_t* pinned_info) {
  if (!have_device()) return nullptr;
  hipStream_t st = (hipStream_t)stream;
  BlobView v;
  std::string err;
  if (!blob_parse(host_blob, &v, &err)) {
    set_error(err);
    return nullptr;
  }
  if (v.scale_dt == DT_DQ8_BNB) {  // double-quantised scales: the synchronous load (own allocation; nothing is left pending)
    ns_weight* ws = ns_hip_weight_from_blob(host_blob, stream);
    if (ws && pinned_info) pinned_info[0] = 0, pinned_info[1] = 0;
    return ws;
  }
  auto pad = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t need = pad(v.q_bytes) + pad(v.s_bytes) + pad(v.z_bytes);
  std::lock_guard<std::mutex> lk(g_mu);
  if (need > g_staging.bytes) {  // grow (a handful of times per model: the largest tensors come early or late, not often)
    if (g_staging.p) {
      hipStreamSynchronize(st);
      hipFree(g_staging.p);
    }
    g_staging.p = nullptr, g_staging.bytes = 0;
    const size_t want = std::max(need + need / 8, size_t(64) << 20);
    if (!hip_ok(hipMalloc((void**)&g_staging.p, want), "hipMalloc(load staging)")) return nullptr;
    g_staging.bytes = want;
  }
  if (!g_staging.info && !hip_ok(hipMalloc((void**)&g_staging.info, size_t(kInfoRing) * 8), "hipMalloc(load info)")) return nullptr;
  const uint8_t* base = static_cast<const uint8_t*>(host_blob);
  uint8_t* dq = g_staging.p;
  uint8_t* ds = dq + pad(v.q_bytes);
  int8_t* dz = v.asym() ? reinterpret_cast<int8_t*>(ds + pad(v.s_bytes)) : nullptr;
  if (!hip_ok(hipMemcpyAsync(dq, base + v.q_off, v.q_bytes, hipMemcpyHostToDevice, st), "H2D codes") ||
      !hip_ok(hipMemcpyAsync(ds, base + v.s_off, v.s_bytes, hipMemcpyHostToDevice, st), "H2D scales") ||
      (dz && !hip_ok(hipMemcpyAsync(dz, base + v.z_off, v.z_bytes, hipMemcpyHostToDevice, st), "H2D zps")))
    return nullptr;
  ns_weight* w = new ns_weight();
  if (!plan_weight(v, w) || !alloc_weight(w, dst, size_t(dst_bytes))) {
    ns_hip_weight_free(w);
    return nullptr;
  }
  RepackArgs ra{dq, ds, dz, v.ntile(), v.packrow(), v.kpad, v.npad, v.cstep, int((v.kpad + v.blocksize - 1) / v.blocksize)};
  ra.src_scale_dt = v.scale_dt;
  uint32_t* dinfo = g_staging.info + 2 * (g_staging.next++ % kInfoRing);
  ra.flags = dinfo + 1;
  bool ok = hip_ok(hipMemsetAsync(dinfo, 0, 8, st), "memset") && hip_ok(launch_repack(ra, w, st), "repack") &&
            (add_native_planes(ra, w, st), true) && hip_ok(launch_scale_absmax(ds, v.s_bytes / (dt_bits(v.scale_dt) / 8), v.scale_dt, dinfo, st, v.cstep, int(v.n)), "scale range") &&
            (w->kind != WK_F8 || hip_ok(launch_scale_spread(ds, v.s_bytes / (dt_bits(v.scale_dt) / 8), v.scale_dt, gemm_f8_scale_drop(w->qtype, v.scale_dt), dinfo, st, v.cstep, int(v.n)), "scale spread")) &&
            hip_ok(hipMemcpyAsync(pinned_info, dinfo, 8, hipMemcpyDeviceToHost, st), "load info D2H");
  if (ok && v.shuf_bytes)
    ok = hip_ok(hipMalloc((void**)&w->shuf, v.shuf_bytes), "hipMalloc(shuffle)") &&
         hip_ok(hipMemcpy(w->shuf, base + v.shuf_off, v.shuf_bytes, hipMemcpyHostToDevice), "H2D shuffle") && check_shuffle(w);
  if (!ok) {
    ns_hip_weight_free(w);
    return nullptr;
  }
  w->load_pending = true;
  return w;
}

int ns_hip_weight_finish_load(ns_weight* w, const uint32_t* info) {
  if (!w || !info) return -1;
  if (!w->load_pending) return 0;  // loaded synchronously (double-quantised scales): nothing to finish
  w->load_pending = false;
  if (info[1] & 1) {  // (bit 1: an fp8 weight whose scale spread keeps it off the tiled GEMM — set_gemm_scale_range)
    w->load_failed = true;
    set_error("F8_E5M2 blob holds codes with exponent field 31 (beyond the reference quantizer's max_norm and fp16)");
    return -1;
  }
  set_gemm_scale_range(w, info[0], (info[1] & 2) != 0);
  return 0;
}

void ns_hip_load_staging_release(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_staging.p) hipFree(g_staging.p);
  if (g_staging.info) hipFree(g_staging.info);
  g_staging = Staging{};
}

int ns_hip_weight_is_external(const ns_weight* w) { return w && w->external ? 1 : 0; }

ns_weight* ns_hip_weight_from_device_blob(const void* dev_blob, size_t blob_bytes, void* stream) {
  if (!have_device()) return nullptr;
  hipStream_t st = (hipStream_t)stream;
  const uint8_t* base = static_cast<const uint8_t*>(dev_blob);
  if (!hip_ok(hipStreamSynchronize(st), "sync before header read")) return nullptr;
  bool io_ok = true;
  BlobIo io = [&](size_t off, void* buf, size_t n, bool) {
    if (off + n > blob_bytes || hipMemcpy(buf, base + off, n, hipMemcpyDeviceToHost) != hipSuccess) {
      memset(buf, 0, n);
      io_ok = false;
    }
  };
  BlobView v;
  std::string err;
  if (!blob_parse_io(io, &v, &err) || !io_ok) {
    set_error(io_ok ? err : "device blob: header read failed");
    return nullptr;
  }
  if (v.size > blob_bytes) {  // (the parser has checked every section against v.size)
    set_error("device blob: the buffer is shorter than the blob's serialized size");
    return nullptr;
  }
  ns_weight* w = weight_from_device_sections(v, base + v.q_off, base + v.s_off,
                                             v.asym() ? (const int8_t*)(base + v.z_off) : nullptr, st,
                                             v.dq_bytes ? reinterpret_cast<const float*>(base + v.dq_off) : nullptr);
  if (w && v.shuf_bytes &&
      (!hip_ok(hipMalloc((void**)&w->shuf, v.shuf_bytes), "hipMalloc(shuffle)") ||
       !hip_ok(hipMemcpy(w->shuf, base + v.shuf_off, v.shuf_bytes, hipMemcpyDeviceToDevice), "D2D shuffle") ||
       !check_shuffle(w))) {
    ns_hip_weight_free(w);
    return nullptr;
  }
  return w;
}

ns_weight* ns_hip_weight_slice(const ns_weight* w, int n0, int n1, int k0, int k1, void* stream) {
  if (!have_device()) return nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (!w || n0 < 0 || n1 > w->n || n0 >= n1 || k0 < 0 || k1 > w->k || k0 >= k1) {
    set_error("slice: range outside the weight");
    return nullptr;
  }
  const int ks = w->kstep_len, bs = w->blocksize;
  const bool per_channel = bs >= w->k;
  if (n0 % 16 != 0 || k0 % ks != 0 || (k1 % ks != 0 && k1 != w->k) ||
      (!per_channel && (k0 % bs != 0 || (k1 % bs != 0 && k1 != w->k)))) {
    set_error("slice: n0 must be a multiple of 16, k0/k1 multiples of the k-step and of the group size");
    return nullptr;
  }
  if (w->shuf && (k0 != 0 || k1 != w->k)) {
    set_error("slice: an activation-shuffle (g_idx) weight cannot be split along K");
    return nullptr;
  }
  ns_weight* o = new ns_weight(*w);
  o->codes = nullptr;
  o->scales = nullptr;
  o->zps = nullptr;
  o->shuf = nullptr;
  o->external = false;      // the slice owns the memory alloc_weight gives it, wherever the parent's lives
  o->load_pending = false;
  o->native = nullptr;  // a slice of a bit-plane weight streams its widened records (no native clone)
  o->n = n1 - n0;
  o->k = k1 - k0;
  o->ntiles = (o->n + 15) / 16;
  o->ksteps = (o->k + ks - 1) / ks;
  const int t0 = n0 / 16, s0 = k0 / ks;
  int r0;  // first scale row
  if (w->sps > 1 || bs == ks) {
    o->srows = o->ksteps;
    r0 = s0;
  } else if (per_channel) {
    o->srows = 1;
    r0 = 0;
    o->blocksize = bs;  // stays "whole K": kernels only test blocksize >= k
  } else {
    o->srows = (o->k + bs - 1) / bs;
    r0 = k0 / bs;
  }
  const int sbytes = dt_bits(w->scale_dt) / 8;
  if (w->interleaved && o->srows != o->ksteps) {
    set_error("slice: layout class changed");
    delete o;
    return nullptr;
  }
  set_strides(o, w->interleaved ? 1 : 0);
  const uint64_t nblk = per_channel ? 1 : (uint64_t(o->k) + bs - 1) / bs;
  o->stream_bytes = uint64_t(o->n) * o->k * dt_bits(o->qtype) / 8 + uint64_t(o->n) * nblk * sbytes +
                    (o->asym ? uint64_t(o->n) * nblk : 0);
  if (!alloc_weight(o)) {
    ns_hip_weight_free(o);
    return nullptr;
  }
  // every array is [tile][row][...]: one strided 2-D copy per array (rows = tiles); interleaved records carry
  // their scales / zero points along
  bool ok = hip_ok(hipMemcpy2DAsync(o->codes, size_t(o->ksteps) * o->qstride,
                                    reinterpret_cast<const uint8_t*>(w->codes) + (size_t(t0) * w->ksteps + s0) * w->qstride,
                                    size_t(w->ksteps) * w->qstride, size_t(o->ksteps) * o->qstride, o->ntiles,
                                    hipMemcpyDeviceToDevice, st), "slice codes");
  if (!o->interleaved) {
    ok = ok && hip_ok(hipMemcpy2DAsync(o->scales, size_t(o->srows) * o->sstride,
                                       static_cast<const uint8_t*>(w->scales) + (size_t(t0) * w->srows + r0) * w->sstride,
                                       size_t(w->srows) * w->sstride, size_t(o->srows) * o->sstride, o->ntiles,
                                       hipMemcpyDeviceToDevice, st), "slice scales");
    if (o->asym)
      ok = ok && hip_ok(hipMemcpy2DAsync(o->zps, size_t(o->srows) * o->zstride,
                                         reinterpret_cast<const uint8_t*>(w->zps) + (size_t(t0) * w->srows + r0) * w->zstride,
                                         size_t(w->srows) * w->zstride, size_t(o->srows) * o->zstride, o->ntiles,
                                         hipMemcpyDeviceToDevice, st), "slice zps");
  }
  if (ok && w->shuf)
    ok = hip_ok(hipMalloc((void**)&o->shuf, size_t(w->k) * sizeof(int)), "hipMalloc(shuffle)") &&
         hip_ok(hipMemcpyAsync(o->shuf, w->shuf, size_t(w->k) * sizeof(int), hipMemcpyDeviceToDevice, st), "slice shuffle");
  if (!ok) {
    ns_hip_weight_free(o);
    return nullptr;
  }
  return o;
}

void ns_hip_weight_free(ns_weight* w) {
  if (!w) return;
  route_invalidate();  // (no plan / window of the device route may keep the weight's device arrays; a later load may be given this address again)
  if (w->codes && !w->external) hipFree(w->codes);  // scales / zps / workspace live in the same allocation
  if (w->shuf) hipFree(w->shuf);
  if (w->native) ns_hip_weight_free(w->native);
  delete w;
}

int ns_hip_weight_info(const ns_weight* w, int* n, int* k, int* bits, int* blocksize, uint64_t* device_bytes) {
  if (!w) return -1;
  if (n) *n = w->n;
  if (k) *k = w->k;
  if (bits) *bits = dt_bits(w->qtype);
  if (blocksize) *blocksize = w->blocksize;
  if (device_bytes) *device_bytes = w->interleaved ? w->codes_bytes : w->codes_bytes + w->scales_bytes + w->zps_bytes;
  return 0;
}

uint64_t ns_hip_weight_stream_bytes(const ns_weight* w) { return w ? w->stream_bytes : 0; }

int ns_hip_set_compute_mode(int mode) {
  if (mode != NS_COMPUTE_FP16 && mode != NS_COMPUTE_REF_INT8) {
    set_error("compute mode: 0 (fp16 activations) or 1 (reference int8 compute)");
    return -1;
  }
  return g_compute_mode.exchange(mode);
}
int ns_hip_get_compute_mode(void) { return g_compute_mode.load(); }

int ns_hip_set_tuning(const char* key, int value) {
  if (key && !strcmp(key, "gemv2")) {
    set_gemv_mode(value);
    return 0;
  }
  if (key && (!strcmp(key, "gvs") || !strcmp(key, "gvs_slices") || !strcmp(key, "gvs_waves") || !strcmp(key, "gvs_grid") || !strcmp(key, "gvs_table") ||
              !strcmp(key, "gvs_finalize"))) {
    set_gemvs_tuning(!strcmp(key, "gvs") ? 0 : !strcmp(key, "gvs_slices") ? 1 : !strcmp(key, "gvs_waves") ? 2 : !strcmp(key, "gvs_grid") ? 3 :
                     !strcmp(key, "gvs_table") ? 4 : 5, value);
    return 0;
  }
  if (key && (!strcmp(key, "moe_gemv_rows") || !strcmp(key, "moe_grouped_rows"))) {  // row thresholds of ns_hip_mul_mat_id's paths; 0 = default, < 0 = off
    set_moe_tuning(!strcmp(key, "moe_gemv_rows") ? 0 : 1, value);
    return 0;
  }
  if (key && !strcmp(key, "g3_min_m")) {
    set_gemm3_min_m(value);
    return 0;
  }
  if (key && !strcmp(key, "i8_tile")) {
    set_i8_tile(value);
    return 0;
  }
  if (key && !strcmp(key, "i8_mfma")) {
    set_i8_mfma_gen(value);
    return 0;
  }
  if (key && !strcmp(key, "attn_heads_first")) {
    set_attn_heads_first(value);
    return 0;
  }
  if (key && !strcmp(key, "g3_wide")) {
    set_gemm3_wide(value);
    return 0;
  }
  if (key && !strcmp(key, "g3_f8")) {  // fp8 weights on the tiled prefill GEMM (1, default) or as before it took them (0); -1: NS_G3_F8 / default
    set_gemm3_f8(value);
    return 0;
  }
  if (key && !strcmp(key, "g3_bm")) {
    set_gemm3_bm(value);
    return 0;
  }
  if (key && !strcmp(key, "gv_nw")) {
    if (value != 0 && value != 2 && value != 4 && value != 8 && value != 16) {
      set_error("ns_hip_set_tuning: gv_nw must be 0, 2, 4, 8 or 16");
      return -1;
    }
    set_decode_waves(value);
    return 0;
  }
  if (key && !strcmp(key, "gv_rows1")) {
    set_gemv_rows1(value);
    return 0;
  }
  if (key && !strcmp(key, "attn_wg_target")) {
    set_attn_tuning(value, 0);
    return 0;
  }
  if (key && !strcmp(key, "attn_min_keys")) {
    set_attn_tuning(0, value);
    return 0;
  }
  if (key && !strcmp(key, "planes")) {
    set_gemv_planes(value);
    return 0;
  }
  if (key && !strcmp(key, "planes_load")) {
    set_planes_load(value);
    return 0;
  }
  if (key && !strcmp(key, "attn_mfma2_rows")) {
    set_attn_mfma2_rows(value);
    return 0;
  }
  if (key && !strcmp(key, "attn_stream_wg_target")) {
    set_attn_stream_tuning(value, 0);
    return 0;
  }
  if (key && !strcmp(key, "attn_stream_min_keys")) {
    set_attn_stream_tuning(0, value);
    return 0;
  }
  if (key && !strcmp(key, "attn_stream")) {
    set_attn_stream(value);
    return 0;
  }
  if (key && !strcmp(key, "attn_inlaunch")) {
    set_attn_inlaunch(value);
    return 0;
  }
  if (key && !strcmp(key, "device_kv_f16")) {  // the device route's attention reads the fp16 mirror of the fp32 kv cache (1, default) or the fp32 cache itself (0); -1: NS_DEVICE_KV
    kv16_set(value);
    return 0;
  }
  set_error("ns_hip_set_tuning: unknown key");
  return -1;
}

int ns_hip_weight_prefetch(const ns_weight* w, uint64_t offset, uint64_t bytes, int workgroups, void* stream) {
  if (!have_device()) return -1;
  if (!w) {
    set_error("prefetch: null weight");
    return -1;
  }
  return hip_ok(launch_prefetch(w, size_t(offset), size_t(bytes), workgroups, (hipStream_t)stream), "prefetch launch") ? 0 : -1;
}

int ns_hip_f32f32_forward(const float* dA, const ns_weight* w, float* dC, int m, int lda, int ldc, int epilogue,
                          const float* dD, int ldd, void* stream) {
  if (!have_device()) return -1;
  return forward_impl(dA, w, dC, m, lda, ldc, epilogue, dD, ldd, (hipStream_t)stream);
}

int ns_hip_fusion_qkv_forward(const float* dA, const ns_weight* wq, const ns_weight* wk, const ns_weight* wv, float* dC,
                              int m, int lda, int ldc, void* stream) {
  return ns_hip_fusion_qkv_forward_h(dA, nullptr, wq, wk, wv, dC, nullptr, m, lda, ldc, stream);
}

int ns_hip_f32f32_forward_h(const float* dA, const void* dA16, const ns_weight* w, float* dC, void* dC16, int m, int lda,
                            int ldc, int epilogue, const float* dD, int ldd, void* stream) {
  return ns_hip_f32f32_forward_x(dA, dA16, w, dC, dC16, m, lda, ldc, epilogue, dD, ldd, nullptr, stream);
}

int ns_hip_f32f32_forward_x(const float* dA, const void* dA16, const ns_weight* w, float* dC, void* dC16, int m, int lda,
                            int ldc, int epilogue, const float* dD, int ldd, const ns_norm_link* link, void* stream) {
  if (!have_device()) return -1;
  return forward_impl(dA, w, dC, m, lda, ldc, epilogue, dD, ldd, (hipStream_t)stream, dA16, dC16, false, link);
}

int ns_hip_norm_prep(int m, int n, const float* dX, int ldx, const float* dGamma, void* dX16, float* dSsq, int ssq_stride,
                     void* stream) {
  if (!have_device()) return -1;
  if (!dX || m < 0 || n < 0 || ldx < n || (dSsq && ssq_stride < (n + 15) / 16)) {
    set_error("norm_prep: invalid argument");
    return -1;
  }
  return hip_ok(launch_norm_prep(m, n, dX, ldx, dGamma, dX16, dSsq, ssq_stride, (hipStream_t)stream), "norm_prep launch") ? 0 : -1;
}

int ns_hip_fusion_qkv_forward_h(const float* dA, const void* dA16, const ns_weight* wq, const ns_weight* wk,
                                const ns_weight* wv, float* dC, void* dC16, int m, int lda, int ldc, void* stream) {
  return ns_hip_fusion_qkv_forward_x(dA, dA16, wq, wk, wv, dC, dC16, m, lda, ldc, nullptr, stream);
}

int ns_hip_warm_up(void) {
  if (!have_device()) return -1;
  static const bool off = getenv("NS_WARM_UP") && atoi(getenv("NS_WARM_UP")) == 0;  // diagnostics
  static std::once_flag once;
  if (!off)
    std::call_once(once, [] {
      touch_gemm_module();
      touch_gemv_module();
      touch_attn_module();
      touch_quant_module();
      ns_hip_reset_error();
    });
  return 0;
}

int ns_hip_rope_cos_sin(int m, int n_past, int n_dims, float freq_base, float freq_scale, float attn_factor,
                        float* dCosSin, void* stream) {
  if (!have_device()) return -1;
  if (m < 0 || n_past < 0 || n_dims < 2 || (n_dims & 1) || !dCosSin) {
    set_error("rope_cos_sin: invalid argument");
    return -1;
  }
  return hip_ok(launch_rope_cos_sin(m, n_past, n_dims, freq_base, freq_scale, attn_factor, dCosSin, (hipStream_t)stream),
                "rope table launch") ? 0 : -1;
}

int ns_hip_rope_cos_sin_mode(int m, int n_past, int n_dims, int mode, float freq_base, float freq_scale, float attn_factor,
                             float* dCosSin, void* stream) {
  // (the arguments are checked before the device is looked for: a refusal touches no device)
  if (mode != 0 && mode != 2) {
    set_error("rope_cos_sin_mode: the table exists for modes 0 (adjacent pairs) and 2 (NeoX)");
    return -1;
  }
  if (m < 0 || n_past < 0 || n_dims < 2 || (n_dims & 1) || !dCosSin) {
    set_error("rope_cos_sin_mode: invalid argument (n_dims even and >= 2)");
    return -1;
  }
  if (mode == 0) return ns_hip_rope_cos_sin(m, n_past, n_dims, freq_base, freq_scale, attn_factor, dCosSin, stream);
  if (!have_device()) return -1;
  return hip_ok(launch_rope_cos_sin(m, n_past, n_dims, freq_base, freq_scale, attn_factor, dCosSin, (hipStream_t)stream, true),
                "rope table launch") ? 0 : -1;
}

int ns_hip_fusion_qkv_rope_forward_x(const float* dA, const void* dA16, const ns_weight* wq, const ns_weight* wk,
                                     const ns_weight* wv, float* dC, int m, int lda, int ldc, const ns_norm_link* link,
                                     const ns_qkv_rope* rope, void* stream) {
  if (!have_device()) return -1;
  if (!wq || !wk || !wv || (!dA && !(dA16 && m > 16)) || !dC || !rope || m < 1) {  // (dA may be NULL at prefill size: fp16-only activations)
    set_error("qkv+rope: null argument");
    return -1;
  }
  if (link && (link->out_gamma || link->out_ssq)) {
    set_error("qkv+rope: the producer side of a norm link needs a single-matrix forward");
    return -1;
  }
  if (rope->flags & ~(NS_QKV_ROPE_KV_CACHE_ONLY | NS_QKV_ROPE_NEOX)) {  // (`flags` is the struct's newest field — a caller built against the older header passes what lay behind it)
    set_error("qkv+rope: unknown bits in ns_qkv_rope::flags (zero the struct before filling it: the field was added in round 5)");
    return -1;
  }
  const bool neox = (rope->flags & NS_QKV_ROPE_NEOX) != 0;
  if (neox != (rope->mode == 2)) {
    // mode 2 without the flag: the unchanged contract (callers keep ns_hip_fusion_qkv_forward_x + ns_hip_rope_qkv_append); the flag says the table is mode 2's
    set_error(neox ? "qkv+rope: NS_QKV_ROPE_NEOX goes with mode 2 only"
                   : "qkv+rope: mode 2 (NeoX) needs NS_QKV_ROPE_NEOX in flags and the table of ns_hip_rope_cos_sin_mode(mode 2); other modes than 0 / 2 have no epilogue");
    return -1;
  }
  if (neox) {
    if (rope->n_dims != rope->head_size || rope->head_size < 32) {
      set_error("qkv+rope (NeoX): whole-head rotation only (n_dims == head_size)");
      return -1;
    }
    if (m <= 16 ? (rope->head_size % 32) != 0 : (rope->head_size != 32 && rope->head_size != 64 && rope->head_size != 128)) {
      set_error(m <= 16 ? "qkv+rope (NeoX) at decode size: head_size must be a multiple of 32 (a workgroup streams both 16-column tiles of a pair)"
                        : "qkv+rope (NeoX) at prefill size: head_size 32, 64 or 128 (a head inside one 128-column block); use ns_hip_fusion_qkv_forward_h + ns_hip_rope_qkv_append for this head size");
      return -1;
    }
  }
  const ns_weight* ws[3] = {wq, wk, wv};
  if (m > 16) {  // prefill size (round 5): the tiled GEMM's fused-QKV launch carries the epilogue; k / v optionally to the cache only
    bool one = !ref_int8_for(wq) && !link && gemm3_takes(wq) && gemm3_takes(wk) && gemm3_takes(wv);
    for (int i = 0; i < 3; i++)
      one &= ws[i]->k == wq->k && ws[i]->kind == wq->kind && ws[i]->blocksize == wq->blocksize && ws[i]->scale_dt == wq->scale_dt &&
             ws[i]->asym == wq->asym && ws[i]->qtype == wq->qtype && !ws[i]->shuf && !ws[i]->load_failed;
    if (one) {
      const bool cache_only = (rope->flags & NS_QKV_ROPE_KV_CACHE_ONLY) != 0;
      SmallMArgs a{};
      a.a = dA, a.a16 = dA16, a.lda = lda, a.m = m, a.ldc = ldc, a.nseg = 3;
      for (int i = 0; i < 3; i++) a.seg[i] = {ws[i], (i == 0 || !cache_only) ? dC + size_t(i) * m * ldc : nullptr, nullptr};
      a.epilogue = NS_EPI_NONE;
      a.rope = rope;
      const hipError_t e = launch_gemm2(a, (hipStream_t)stream);
      if (e != hipErrorNotSupported) return hip_ok(e, "qkv+rope GEMM launch") ? 0 : -1;
    }
    if (getenv("NS_ROPE_GEMM_DEBUG")) fprintf(stderr, "qkv+rope at prefill size refused: one format %d, m %d, k %d, n %d %d %d, head_size %d, ldc %d\n", int(one), m, wq->k, wq->n, wk->n, wv->n, rope->head_size, ldc);
    set_error("qkv+rope at prefill size: needs three weights of one format the tiled kernel takes (integer, f4, or fp8 with the g3_f8 switch on), plain whole-head RoPE, head_size a multiple of 4, matrix widths multiples of 128, 16-byte aligned outputs and no norm link");
    return -1;
  }
  bool same = !ref_int8_for(wq) && m <= 16 && dA16;
  for (int i = 0; i < 3; i++)
    same &= ws[i]->k == wq->k && ws[i]->kind == wq->kind && ws[i]->blocksize == wq->blocksize &&
            ws[i]->scale_dt == wq->scale_dt && ws[i]->asym == wq->asym && ws[i]->qtype == wq->qtype && !ws[i]->shuf;
  if (!same || !smallm_supported(wq, m)) {
    set_error("qkv+rope: needs three weights of one format, m <= 16, the fp16 shadow of A and the fp16 compute mode");
    return -1;
  }
  SmallMArgs a{};
  a.a = dA;
  a.a16 = dA16;
  a.lda = lda;
  a.m = m;
  a.ldc = ldc;
  a.nseg = 3;
  for (int i = 0; i < 3; i++) a.seg[i] = {ws[i], dC + size_t(i) * m * ldc, nullptr};
  a.epilogue = NS_EPI_NONE;
  a.link = link;
  a.rope = rope;
  return hip_ok(launch_smallm(a, (hipStream_t)stream), "qkv+rope launch") ? 0 : -1;
}

int ns_hip_fusion_qkv_forward_x(const float* dA, const void* dA16, const ns_weight* wq, const ns_weight* wk,
                                const ns_weight* wv, float* dC, void* dC16, int m, int lda, int ldc,
                                const ns_norm_link* link, void* stream) {
  if (!have_device()) return -1;
  if (!wq || !wk || !wv) {
    set_error("qkv: null weight");
    return -1;
  }
  const ns_weight* ws[3] = {wq, wk, wv};
  bool same = true;
  for (int i = 1; i < 3; i++)
    same &= ws[i]->k == wq->k && ws[i]->kind == wq->kind && ws[i]->blocksize == wq->blocksize &&
            ws[i]->scale_dt == wq->scale_dt && ws[i]->asym == wq->asym && ws[i]->qtype == wq->qtype;
  same &= !wq->shuf && !wk->shuf && !wv->shuf;  // each shuffled weight gathers its own A' (unfused path)
  same &= !ref_int8_for(wq);                    // int8-reference mode: three plain forwards share nothing but A
  hipStream_t st = (hipStream_t)stream;
  if (link && (link->out_gamma || link->out_ssq)) {
    set_error("qkv: the producer side of a norm link needs a single-matrix forward");
    return -1;
  }
  if (link && !link_ok(link, wq, m, dA16)) return -1;
  if (ref_int8_for(wq) && m <= 4 && !link) {  // int8-reference numerics, decode-sized: ONE activation quantization + one launch
    bool same8 = true;
    for (int i = 1; i < 3; i++)
      same8 &= ref_int8_for(ws[i]) && ws[i]->k == wq->k && ws[i]->kind == wq->kind && ws[i]->blocksize == wq->blocksize &&
               ws[i]->scale_dt == wq->scale_dt && ws[i]->asym == wq->asym && ws[i]->qtype == wq->qtype;
    same8 &= !wq->shuf && !wk->shuf && !wv->shuf;
    I8Act q;
    if (same8 && i8_quantize_for_decode(dA, lda, wq, m, st, false, &q) == hipSuccess) {
      SmallMArgs a{};
      a.a = dA, a.lda = lda, a.m = m, a.ldc = ldc, a.nseg = 3;
      for (int i = 0; i < 3; i++)
        a.seg[i] = {ws[i], dC + size_t(i) * m * ldc, dC16 ? static_cast<uint16_t*>(dC16) + size_t(i) * m * ldc : nullptr};
      a.epilogue = NS_EPI_NONE;
      a.i8 = &q;
      const hipError_t e = launch_gemv_i8(a, &q, st);
      if (e == hipSuccess) return 0;
      if (e != hipErrorNotSupported) return hip_ok(e, "int8-reference qkv launch") ? 0 : -1;
    }
  }
  if (same && m > 64 && !link) {  // GEMM size: the three matrices side by side in ONE launch of the tiled kernel
    SmallMArgs a{};
    a.a = dA;
    a.a16 = dA16;
    a.lda = lda;
    a.m = m;
    a.ldc = ldc;
    a.nseg = 3;
    for (int i = 0; i < 3; i++)
      a.seg[i] = {ws[i], dC + size_t(i) * m * ldc, dC16 ? static_cast<uint16_t*>(dC16) + size_t(i) * m * ldc : nullptr};
    a.epilogue = NS_EPI_NONE;
    const hipError_t e = launch_gemm2(a, st);
    if (e == hipSuccess) return 0;
    if (e != hipErrorNotSupported) return hip_ok(e, "qkv GEMM launch") ? 0 : -1;
  }
  if (!same || m > 64) {  // fall back to three launches (still on the GPU)
    // int8-reference mode: the three weights share one activation quantization when K and the group size agree
    auto same_aq = [&](int i) {
      return i > 0 && ref_int8_for(ws[i]) && ref_int8_for(ws[0]) && ws[i]->k == ws[0]->k &&
             ws[i]->blocksize == ws[0]->blocksize && !ws[i]->shuf && !ws[0]->shuf;
    };
    for (int i = 0; i < 3; i++)
      if (forward_impl(dA, ws[i], dC + size_t(i) * m * ldc, m, lda, ldc, NS_EPI_NONE, nullptr, 0, st, dA16,
                       dC16 ? static_cast<uint16_t*>(dC16) + size_t(i) * m * ldc : nullptr, same_aq(i), link))
        return -1;
    return 0;
  }
  SmallMArgs a{};
  a.a = dA;
  a.a16 = dA16;
  a.lda = lda;
  a.m = m;
  a.ldc = ldc;
  a.nseg = 3;
  for (int i = 0; i < 3; i++)  // ip_fusion_qkv.cpp:84-86
    a.seg[i] = {ws[i], dC + size_t(i) * m * ldc, dC16 ? static_cast<uint16_t*>(dC16) + size_t(i) * m * ldc : nullptr};
  a.epilogue = NS_EPI_NONE;
  a.link = link;
  return hip_ok(launch_smallm(a, st), "qkv launch") ? 0 : -1;
}

int ns_hip_fusion_ffn3_gateup(const float* dA, const ns_weight* w1, const ns_weight* w3, float* dTmp1, float* dTmp2,
                              int seq, int act, void* stream) {
  return ns_hip_fusion_ffn3_gateup_h(dA, nullptr, w1, w3, dTmp1, dTmp2, nullptr, seq, act, stream);
}

int ns_hip_fusion_ffn3_gateup_h(const float* dA, const void* dA16, const ns_weight* w1, const ns_weight* w3,
                                float* dTmp1, float* dTmp2, void* dTmp2_16, int seq, int act, void* stream) {
  return ns_hip_fusion_ffn3_gateup_x(dA, dA16, w1, w3, dTmp1, dTmp2, dTmp2_16, seq, act, nullptr, stream);
}

int ns_hip_fusion_ffn3_gateup_x(const float* dA, const void* dA16, const ns_weight* w1, const ns_weight* w3,
                                float* dTmp1, float* dTmp2, void* dTmp2_16, int seq, int act, const ns_norm_link* link,
                                void* stream) {
  if (!have_device()) return -1;
  if (!w1 || !w3 || (!dTmp2 && !dTmp2_16) || (!dA && !dA16)) {  // (dA may be NULL at GEMM size: fp16-only activations, as for the single forward)
    set_error("ffn3 gate/up: null argument");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int fin = w1->k, fmid = w1->n;
  const bool same = w3->k == fin && w3->n == fmid && w3->kind == w1->kind && w3->blocksize == w1->blocksize &&
                    w3->scale_dt == w1->scale_dt && w3->asym == w1->asym && w3->qtype == w1->qtype && !w1->shuf &&
                    !w3->shuf;
  const bool ref8 = ref_int8_for(w1);  // int8-reference mode: the two GEMVs and the activation stay separate operators
  // GEMM size (round 5): ONE launch of the tiled kernel on gate / up tile pairs — act(A W1) * (A W3) is formed in registers, so
  // neither tmp1 nor an fp32 tmp2 has to exist (each is written only if the caller hands a pointer: the reference's graph treats
  // both as scratch, ne_layers.c:2573-2576); before, W1 wrote tmp1 (fp32), W3 read it back and wrote tmp2 (fp32 + fp16)
  // (fp8 weights: from 65 rows; from 17 like the rest only where nothing else serves the call — fp16-only activations)
  const bool f8_rows = w1->kind != WK_F8 || (gemm3_takes(w1) && gemm3_takes(w3) && (seq > 64 || !dA));
  if (same && !ref8 && !link && seq > 16 && (seq > 64 || seq >= tiled_from_rows(w1)) && f8_rows && (dTmp2 || dTmp2_16) &&
      smallm_supported(w1, seq)) {
    SmallMArgs a{};
    a.a = dA, a.a16 = dA16, a.lda = fin, a.m = seq, a.ldc = fmid, a.nseg = 2;
    a.seg[0] = {w1, dTmp2, dTmp2_16};
    a.seg[1] = {w3, dTmp2, nullptr};
    a.epilogue = act;
    a.dual = true;
    a.c2 = dTmp1;
    const hipError_t e = launch_gemm2(a, st);
    if (e == hipSuccess) return 0;
    if (e != hipErrorNotSupported) return hip_ok(e, "ffn gate/up GEMM launch") ? 0 : -1;
  }
  if (!dA) {
    set_error("ffn3 gate/up: fp16-only activations need the tiled kernel's fused launch (matching formats, more than 16 rows, K a multiple of 64, 16-byte aligned)");
    return -1;
  }
  if (!dTmp2) {  // the paths below produce the fp32 product
    dTmp2 = static_cast<float*>(stream_scratch(st, size_t(seq) * fmid * 4, 9));
    if (!dTmp2) {
      set_error("ffn3 gate/up: no scratch for tmp2 (out of device memory)");
      return -1;
    }
  }
  if (same && smallm_dual_ok(seq) && smallm_supported(w1, seq) && !ref8) {
    SmallMArgs a{};
    a.a = dA;
    a.a16 = dA16;
    a.lda = fin;
    a.m = seq;
    a.ldc = fmid;
    a.nseg = 2;
    a.seg[0] = {w1, dTmp2, dTmp2_16};
    a.seg[1] = {w3, dTmp2, nullptr};
    a.epilogue = act;
    a.dual = true;
    a.c2 = dTmp1;
    a.link = link;
    if (link && ((link->out_gamma || link->out_ssq) || !link_ok(link, w1, seq, dA16))) {
      if (link->out_gamma || link->out_ssq) set_error("ffn gate/up: the producer side of a norm link needs a single-matrix forward");
      return -1;
    }
    return hip_ok(launch_smallm(a, st), "ffn gate/up launch") ? 0 : -1;
  }
  if (link) {
    set_error("ffn gate/up: a norm link needs the fused launch (matching formats, seq <= 16)");
    return -1;
  }
  if (ref8 && same && seq <= 4 && ref_int8_for(w3)) {  // int8-reference numerics, decode-sized: one quantization, one launch
    I8Act q;
    if (i8_quantize_for_decode(dA, fin, w1, seq, st, false, &q) == hipSuccess) {
      SmallMArgs a{};
      a.a = dA, a.lda = fin, a.m = seq, a.ldc = fmid, a.nseg = 2;
      a.seg[0] = {w1, dTmp2, dTmp2_16};
      a.seg[1] = {w3, dTmp2, nullptr};
      a.epilogue = act;
      a.dual = true;
      a.c2 = dTmp1;
      a.i8 = &q;
      const hipError_t e = launch_gemv_i8(a, &q, st);
      if (e == hipSuccess) return 0;
      if (e != hipErrorNotSupported) return hip_ok(e, "int8-reference gate/up launch") ? 0 : -1;
    }
  }
  if (!dTmp1) dTmp1 = static_cast<float*>(stream_scratch(st, size_t(seq) * fmid * 4, 5));
  if (!dTmp1) {
    set_error("ffn3: no scratch for tmp1 on the unfused path (out of device memory)");
    return -1;
  }
  if (forward_impl(dA, w1, dTmp1, seq, fin, fmid, act, nullptr, 0, st, dA16, nullptr)) return -1;
  const bool same_aq = ref8 && ref_int8_for(w3) && w3->k == w1->k && w3->blocksize == w1->blocksize && !w1->shuf && !w3->shuf;
  return forward_impl(dA, w3, dTmp2, seq, fin, fmid, NS_EPI_MUL, dTmp1, fmid, st, dA16, dTmp2_16, same_aq);
}

int ns_hip_fusion_ffn3_forward(const float* dA, const ns_weight* w1, const ns_weight* w2, const ns_weight* w3,
                               float* dTmp1, float* dTmp2, float* dOut, int seq, int act, void* stream) {
  if (!have_device()) return -1;
  return ns_hip_fusion_ffn3_forward_h(dA, nullptr, w1, w2, w3, dTmp1, dTmp2, nullptr, dOut, nullptr, seq, act, stream);
}

int ns_hip_fusion_ffn3_forward_h(const float* dA, const void* dA16, const ns_weight* w1, const ns_weight* w2,
                                 const ns_weight* w3, float* dTmp1, float* dTmp2, void* dTmp2_16, float* dOut,
                                 void* dOut16, int seq, int act, void* stream) {
  if (!have_device()) return -1;
  if (!w1 || !w2 || !w3 || w2->k != w1->n) {
    set_error("ffn3: bad argument");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int fmid = w1->n;
  // GEMM size, no fp32 tmp2 asked for: the intermediate exists as fp16 only (the down projection multiplies fp16 activations anyway);
  // it lives in the caller's dTmp2_16 or in per-stream scratch
  if (!dTmp2 && seq > 16 && !w2->shuf && !ref_int8_for(w2) && (w2->kind != WK_F8 || (gemm3_takes(w2) && (seq > 64 || !dA))) && fmid % 64 == 0) {
    void* t16 = dTmp2_16 ? dTmp2_16 : stream_scratch(st, size_t(seq) * fmid * 2, 8);
    if (t16 && ns_hip_fusion_ffn3_gateup_h(dA, dA16, w1, w3, dTmp1, nullptr, t16, seq, act, stream) == 0) {
      SmallMArgs a{};
      a.a = nullptr, a.a16 = t16, a.lda = fmid, a.m = seq, a.ldc = w2->n, a.nseg = 1;
      a.seg[0] = {w2, dOut, dOut16};
      a.epilogue = NS_EPI_NONE;
      const hipError_t e = launch_gemm2(a, st);
      if (e == hipSuccess) return 0;
      if (e != hipErrorNotSupported) return hip_ok(e, "ffn down GEMM launch") ? 0 : -1;
    }
    // (outside the tiled kernel's envelope: the general path below, on an fp32 intermediate)
  }
  if (!dTmp2) dTmp2 = static_cast<float*>(stream_scratch(st, size_t(seq) * fmid * 4, 9));
  if (!dTmp2) {
    set_error("ffn3: no scratch for tmp2 (out of device memory)");
    return -1;
  }
  if (ns_hip_fusion_ffn3_gateup_h(dA, dA16, w1, w3, dTmp1, dTmp2, dTmp2_16, seq, act, stream)) return -1;
  return forward_impl(dTmp2, w2, dOut, seq, w1->n, w2->n, NS_EPI_NONE, nullptr, 0, st, dTmp2_16, dOut16);
}

int ns_hip_fusion_ffn2_forward(const float* dA, const ns_weight* w1, const ns_weight* w2, const float* dB1,
                               const float* dB2, float* dTmp1, float* dOut, int seq, bool broadcast_bias, void* stream) {
  if (!have_device()) return -1;
  if (!w1 || !w2 || !dTmp1) {
    set_error("ffn2: null argument");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int fin = w1->k, fmid = w1->n, fout = w2->n;
  if (forward_impl(dA, w1, dTmp1, seq, fin, fmid, dB1 ? NS_EPI_ADD_GELU : NS_EPI_GELU, dB1, broadcast_bias ? 0 : fmid, st))
    return -1;
  return forward_impl(dTmp1, w2, dOut, seq, fmid, fout, dB2 ? NS_EPI_ADD : NS_EPI_NONE, dB2, broadcast_bias ? 0 : fout, st);
}

int ns_hip_quantize_fp_u8_colblock(int row, int col, const float* dSrc, int ld_src, uint8_t* dDst, int ld_dst,
                                   float* dScales, int ld_scale, uint8_t* dZps, int blocksize, float* dBlkReduce,
                                   void* stream) {
  if (!have_device()) return -1;
  if (!dSrc || !dDst || !dScales || !dZps || row < 0 || col < 0 || blocksize <= 0) {
    set_error("quantize_fp_u8_colblock: invalid argument");
    return -1;
  }
  if (!dBlkReduce && row >= 16) {  // GEMM-sized, no block sums wanted: the vector form (bit-identical codes, scales, zero points)
    const hipError_t e = launch_aquant_u8_vec(row, col, dSrc, ld_src, dDst, ld_dst, dScales, ld_scale, dZps, blocksize, nullptr, 0,
                                              false, (hipStream_t)stream);
    if (e != hipErrorNotSupported) return hip_ok(e, "activation quantize launch") ? 0 : -1;
  }
  return hip_ok(launch_aquant_u8(row, col, dSrc, ld_src, dDst, ld_dst, dScales, ld_scale, dZps, blocksize, dBlkReduce,
                                 (hipStream_t)stream), "activation quantize launch") ? 0 : -1;
}

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

void* bestla_get_thread_handle(void) { return &g_cache; }

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
// storage record of bestla_device_load_storage, not a blob (first word all ones: no blob starts like that, csrc/ns_device.hip DeviceStorage) — refused
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
    if (w->n != _n || w->k != _k || w->kind != q->kind || w->blocksize != q->blocksize || w->scale_dt != q->scale_dt ||
        w->asym != q->asym || w->qtype != q->qtype)
      return false;
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

// device-pointer twins of the three element-wise operators (precedent: bestla_device_rms_norm_f32 / _mul_f32 / _add_f32,
// ne_bestla.h:99-105): same arithmetic, asynchronous on `stream`, capturable
int ns_hip_layernormalization(int norm_count, int norm_size, bool isrms, float epsilon, const float* dIn, float* dOut,
                              void* stream) {
  if (!have_device()) return -1;
  if (!dIn || !dOut || norm_count < 0 || norm_size <= 0) {
    set_error("layernormalization: invalid argument");
    return -1;
  }
  return hip_ok(launch_rmsnorm(norm_count, norm_size, isrms, epsilon, dIn, dOut, (hipStream_t)stream), "norm launch") ? 0 : -1;
}
int ns_hip_norm_mul_h(int norm_count, int norm_size, bool isrms, float epsilon, const float* dIn, const float* dGamma,
                      float* dOut, void* dOut16, void* stream) {
  if (!have_device()) return -1;
  if (!dIn || (!dOut && !dOut16) || norm_count < 0 || norm_size <= 0) {  // (dOut may be NULL: the fp16 shadow alone)
    set_error("norm_mul: invalid argument");
    return -1;
  }
  return hip_ok(launch_rmsnorm(norm_count, norm_size, isrms, epsilon, dIn, dOut, (hipStream_t)stream, dGamma, dOut16),
                "norm launch") ? 0 : -1;
}
int ns_hip_rope_f32(const float* dSrc, float* dDst, int batch, int seq, int heads, int head_size, int n_past, int n_dims,
                    int mode, float freq_base, float freq_scale, float ext_factor, float attn_factor, void* stream) {
  if (!have_device()) return -1;
  if (route_hook(stream)) {  // the reference's device route: described, verified against the plan, replayed (ns_route.cpp)
    RouteOp op;
    memset(&op, 0, sizeof(op));
    op.kind = RK_ROPE, op.p[0] = dSrc, op.p[1] = dDst;
    op.i[0] = batch, op.i[1] = seq, op.i[2] = heads, op.i[3] = head_size, op.i[4] = n_past, op.i[5] = n_dims, op.i[6] = mode;
    op.f[0] = freq_base, op.f[1] = freq_scale, op.f[2] = ext_factor, op.f[3] = attn_factor;
    return route_submit(op);
  }
  if (!dSrc || !dDst || batch < 0 || seq < 0 || heads < 0 || head_size <= 0 || (head_size & 1) || n_dims <= 0 ||
      (n_dims & 1) || n_dims > head_size || n_past < 0) {
    set_error("rope: invalid argument");
    return -1;
  }
  if ((mode & ~2) != 0 || ext_factor != 0.f) {
    set_error("rope: this entry takes modes 0 and 2 (NeoX) without YaRN extrapolation (GLM: ns_hip_rope_f32_glm, YaRN / long-rope: their own entries; shift is asserted against by the reference itself)");
    return -1;
  }
  return hip_ok(launch_rope(dSrc, dDst, batch, seq, heads, head_size, n_past, n_dims, mode, freq_base, freq_scale, attn_factor,
                            (hipStream_t)stream), "rope launch") ? 0 : -1;
}
// GLM branch (mode & 4) of ne_compute_forward_rope_f32, ne_layers.c:9317-9347
int ns_hip_rope_f32_glm(const float* dSrc, float* dDst, int batch, int seq, int heads, int head_size, int n_past, int n_dims,
                        int mode, float freq_base, int prompt_size, const int* n_padding, void* stream) {
  if (!have_device()) return -1;
  if (!dSrc || !dDst || !n_padding || batch < 0 || batch > 32 || seq < 0 || heads < 0 || head_size <= 0 || (head_size & 3) ||
      n_dims <= 0 || (n_dims & 1) || n_past < 0 || n_dims / 2 * 3 + head_size / 4 > head_size) {
    set_error("rope (GLM): invalid argument (head_size % 4 == 0, 3 n_dims / 2 + head_size / 4 <= head_size, batch <= 32)");
    return -1;
  }
  if (!(mode & 4) || (mode & ~5) != 0) {
    set_error("rope (GLM): mode must be 4 (or 5 = 4 | skip)");
    return -1;
  }
  return hip_ok(launch_rope_glm(dSrc, dDst, batch, seq, heads, head_size, n_past, n_dims, (mode & 1) != 0, freq_base,
                                prompt_size, n_padding, (hipStream_t)stream), "rope (GLM) launch") ? 0 : -1;
}
// ne_compute_forward_rope_f32 with the YaRN extrapolation mix (ext_factor != 0): corr_dims from
// ggml_rope_yarn_corr_dims (ne_layers.c:9219-9231) and the magnitude correction of rope_yarn (:9210) are evaluated here
// with the host libm, exactly where the reference evaluates them.
static int rope_ext(const float* dSrc, float* dDst, int batch, int seq, int heads, int head_size, int n_past, int n_dims,
                    int mode, float freq_base, float freq_scale, int n_orig_ctx, float ext_factor, float attn_factor,
                    float beta_fast, float beta_slow, const float* dFactors, float scale_factor, void* stream) {
  if (!have_device()) return -1;
  if (!dSrc || !dDst || batch < 0 || seq < 0 || heads < 0 || head_size <= 0 || (head_size & 1) || n_dims <= 0 ||
      (n_dims & 1) || n_dims > head_size || n_past < 0 || !(freq_scale > 0.f)) {
    set_error("rope: invalid argument");
    return -1;
  }
  const bool longrope = (mode & 0x10) != 0;
  if ((mode & ~(2 | 8 | 0x10)) != 0 || (longrope && !dFactors)) {  // bit 3 ("use_yarn") carries no arithmetic in the reference
    set_error("rope: modes 0, 2 (NeoX) and 0x10 (long-rope, needs the factor array) are implemented (no GLM / shift)");
    return -1;
  }
  float corr0 = 0.f, corr1 = 0.f, mscale = attn_factor;
  if (ext_factor != 0.f) {
    auto corr_dim = [&](float n_rot) {
      return n_dims * logf(n_orig_ctx / (n_rot * 2 * (float)3.14159265358979323846)) / (2 * logf(freq_base));
    };
    corr0 = std::max(0.f, floorf(corr_dim(beta_fast)));
    corr1 = std::min(float(n_dims - 1), ceilf(corr_dim(beta_slow)));
    mscale *= 1.0f + 0.1f * logf(1.0f / freq_scale);
  }
  // the long-rope branch walks the row like the NeoX one (ne_layers.c:9349-9377)
  return hip_ok(launch_rope(dSrc, dDst, batch, seq, heads, head_size, n_past, n_dims, longrope ? 2 : (mode & 2), freq_base,
                            freq_scale, mscale, (hipStream_t)stream, ext_factor, corr0, corr1, longrope ? dFactors : nullptr,
                            scale_factor), "rope launch") ? 0 : -1;
}
// ne_compute_forward_rope_f32 with the YaRN extrapolation mix (ext_factor != 0): corr_dims from
// ggml_rope_yarn_corr_dims (ne_layers.c:9219-9231) and the magnitude correction of rope_yarn (:9210) are evaluated on
// the host with its libm, exactly where the reference evaluates them.
int ns_hip_rope_f32_yarn(const float* dSrc, float* dDst, int batch, int seq, int heads, int head_size, int n_past,
                         int n_dims, int mode, float freq_base, float freq_scale, int n_orig_ctx, float ext_factor,
                         float attn_factor, float beta_fast, float beta_slow, void* stream) {
  if (route_hook(stream)) {
    RouteOp op;
    memset(&op, 0, sizeof(op));
    op.kind = RK_ROPE_YARN, op.p[0] = dSrc, op.p[1] = dDst;
    op.i[0] = batch, op.i[1] = seq, op.i[2] = heads, op.i[3] = head_size, op.i[4] = n_past, op.i[5] = n_dims, op.i[6] = mode, op.i[7] = n_orig_ctx;
    op.f[0] = freq_base, op.f[1] = freq_scale, op.f[2] = ext_factor, op.f[3] = attn_factor, op.f[4] = beta_fast, op.f[5] = beta_slow;
    return route_submit(op);
  }
  if (mode & 0x10) {
    set_error("rope: long-rope needs ns_hip_rope_f32_longrope (factor array)");
    return -1;
  }
  return rope_ext(dSrc, dDst, batch, seq, heads, head_size, n_past, n_dims, mode, freq_base, freq_scale, n_orig_ctx, ext_factor,
                  attn_factor, beta_fast, beta_slow, nullptr, 1.f, stream);
}
// long-rope (mode bit 0x10, phi-3 style; ne_layers.c:9349-9377): theta / dFactors[pair] before rope_yarn, cos and sin
// times scale_factor; dFactors is a device array of n_dims / 2 floats (the graph's dst->opt[1])
int ns_hip_rope_f32_longrope(const float* dSrc, float* dDst, int batch, int seq, int heads, int head_size, int n_past,
                             int n_dims, float freq_base, float freq_scale, int n_orig_ctx, float ext_factor,
                             float attn_factor, float beta_fast, float beta_slow, const float* dFactors,
                             float scale_factor, void* stream) {
  return rope_ext(dSrc, dDst, batch, seq, heads, head_size, n_past, n_dims, 0x10, freq_base, freq_scale, n_orig_ctx, ext_factor,
                  attn_factor, beta_fast, beta_slow, dFactors, scale_factor, stream);
}

int ns_hip_rope_qkv_append(float* dQ, const float* dK, const float* dV, void* dKcache16, void* dVcache16, int seq, int heads,
                           int heads_kv, int head_size, int n_past, int n_dims, int mode, float freq_base, float freq_scale,
                           float ext_factor, float attn_factor, long long cache_step_sl, long long cache_step_head,
                           void* stream) {
  if (!have_device()) return -1;
  if (!dQ || !dK || !dV || !dKcache16 || !dVcache16 || seq < 0 || heads <= 0 || heads_kv <= 0 || head_size <= 0 ||
      (head_size & 1) || n_dims <= 0 || (n_dims & 1) || n_dims > head_size || n_past < 0) {
    set_error("rope_qkv_append: invalid argument");
    return -1;
  }
  if ((mode & ~2) != 0 || ext_factor != 0.f || ((mode & 2) && head_size % n_dims != 0)) {
    set_error("rope_qkv_append: only modes 0 and 2 (NeoX, head_size a multiple of n_dims) without YaRN extrapolation");
    return -1;
  }
  return hip_ok(launch_rope_qkv_append(dQ, dK, dV, dKcache16, dVcache16, seq, heads, heads_kv, head_size, n_past, n_dims, mode,
                                       freq_base, freq_scale, attn_factor, cache_step_sl, cache_step_head,
                                       (hipStream_t)stream), "rope/kv-append launch") ? 0 : -1;
}
// device twins of bestla_device_elewise_f32 (NE_OP_SILU) and bestla_device_dup_f32 (ne_bestla.h:103-109)
int ns_hip_silu_f32(const float* dSrc, float* dDst, size_t n, void* stream) {
  if (!have_device()) return -1;
  if (n && (!dSrc || !dDst)) {
    set_error("silu: null argument");
    return -1;
  }
  return hip_ok(launch_silu(dSrc, dDst, n, (hipStream_t)stream), "silu launch") ? 0 : -1;
}
int ns_hip_dup_f32(const float* dSrc, void* dDst, const long long ne[4], const long long src_nb[4],
                   const long long dst_nb[4], bool dst_is_f16, void* stream) {
  if (!have_device()) return -1;
  if (!dSrc || !dDst || !ne || !src_nb || !dst_nb) {
    set_error("dup: null argument");
    return -1;
  }
  for (int i = 0; i < 4; i++)
    if (ne[i] < 0) {
      set_error("dup: negative extent");
      return -1;
    }
  if (route_hook(stream)) {
    RouteOp op;
    memset(&op, 0, sizeof(op));
    op.kind = RK_DUP, op.p[0] = dSrc, op.p[1] = dDst;
    for (int i = 0; i < 4; i++) op.i[i] = ne[i], op.i[4 + i] = src_nb[i], op.i[8 + i] = dst_nb[i];
    op.i[12] = dst_is_f16 ? 1 : 0;
    return route_submit(op);
  }
  return hip_ok(launch_dup(dSrc, dDst, ne, src_nb, dst_nb, dst_is_f16, (hipStream_t)stream), "dup launch") ? 0 : -1;
}

int ns_hip_mul(int batch, int vsize, const float* dTensor, const float* dVector, int vstep, float* dOut, void* stream) {
  if (!have_device()) return -1;
  if (!dTensor || !dVector || !dOut || batch < 0 || vsize <= 0) {
    set_error("mul: invalid argument");
    return -1;
  }
  return hip_ok(launch_bcast_binary(batch, vsize, dTensor, dVector, vstep, dOut, true, (hipStream_t)stream), "mul launch") ? 0 : -1;
}
int ns_hip_add(int batch, int vsize, const float* dTensor, const float* dVector, int vstep, float* dOut, void* stream) {
  if (!have_device()) return -1;
  if (!dTensor || !dVector || !dOut || batch < 0 || vsize <= 0) {
    set_error("add: invalid argument");
    return -1;
  }
  return hip_ok(launch_bcast_binary(batch, vsize, dTensor, dVector, vstep, dOut, false, (hipStream_t)stream), "add launch") ? 0 : -1;
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
