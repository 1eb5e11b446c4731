// ns_weights.cpp — blob -> device weight: the load, slice and free of weights (ns_hip_weight_*) and the cache behind the host-pointer
// entries.
//
// Unlike the reference, which re-parses the blob header (heap alloc + delete) on every call
// (neural_speed/core/layers/bestla_gemm.cpp:514/:617), a blob pointer is parsed once: the first forward that sees it re-lays the
// weight out for MI355X in HBM and caches blob pointer -> device weight.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "ns_api_int.h"

using namespace ns;  // NOLINT

namespace {
std::mutex g_mu;
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
size_t g_cache_bytes = 0;
}  // namespace
ns::CachePin::CachePin() {
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_pin_count++ == 0) g_pin_floor = g_cache_tick;
}
ns::CachePin::~CachePin() {
  std::lock_guard<std::mutex> lk(g_mu);
  --g_pin_count;
}
namespace {
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
std::atomic<int> g_planes_load{-1};
}  // namespace
void ns::set_planes_load(int on) { g_planes_load.store(on != 0); }
namespace {
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

}  // namespace

ns_weight* ns::cached_weight(const void* blob) {
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

extern "C" {

void ns_hip_cache_clear(void) {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& kv : g_cache) ns_hip_weight_free(kv.second.w);
    g_cache.clear();
    g_cache_bytes = 0;
  }
  kv_mirrors_clear();  // ns_kvcache.hip: device mirrors of library-managed kv caches
}

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

}  // extern "C"
