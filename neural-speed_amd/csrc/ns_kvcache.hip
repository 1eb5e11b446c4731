// ns_kvcache.hip — the library-managed kv-cache of the reference's mha_dense C surface (bestla_reordered_attn_*, bestla_fusion_attn_fp32_batch_cpy_*)
// and the host-tensor attention entry: fp16 cache rows, device mirrors of the caches the graph keeps in host memory, staging of host tensors.
// The attention itself is ns_attn.cpp's device entry.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "ns_attn.h"

namespace ns {

// ---- library-managed ("reordered") kv-cache, MI355X form: plain fp16 [batch][head][seq_max][head_size] -----------------
// The reference hands the cache to BesTLA as an opaque buffer (sizes / strides from bestla_reordered_attn_fp32_batch_kv_info,
// contents only through the update / shift / copy / forward entries, mha_dense.h:124-172) and packs it for AMX / AVX tiles.
// Nothing but this module looks inside, so the layout here is the one the attention kernels stream best.
// slab (optional): the device mirror of the cache, rows seq_off .. of every (batch, head) slab of seq_max rows
__global__ void kv_update_kernel(const float* __restrict__ src, _Float16* __restrict__ out, int batch, int heads, int hs,
                                 int seq, long long step_bs, long long step_head, long long step_seq, long long step_hs,
                                 _Float16* __restrict__ slab = nullptr, int seq_max = 0, int seq_off = 0) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t total = size_t(batch) * heads * seq * hs;
  if (gid >= total) return;
  const int j = int(gid % hs);
  const int i = int((gid / hs) % seq);
  const int h = int((gid / (size_t(hs) * seq)) % heads);
  const int b = int(gid / (size_t(hs) * seq * heads));
  const _Float16 v = (_Float16)src[b * step_bs + h * step_head + i * step_seq + j * step_hs];
  out[gid] = v;  // out: [batch][head][seq][hs]
  if (slab) slab[((size_t(b) * heads + h) * seq_max + seq_off + i) * hs + j] = v;
}
// rows [seq_keep, seq_max) of every (batch, head): adjacent pairs rotated by the one angle set in cossin = {cos_0, sin_0,
// cos_1, sin_1, ...} (fp16), as ne_compute_forward_rope_bestla prepares it (ne_layers.c:9636-9651)
__global__ void kv_shift_rope_kernel(_Float16* __restrict__ rows, const _Float16* __restrict__ cossin, size_t nrows, int hs) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int half = hs / 2;
  if (gid >= nrows * half) return;
  const size_t r = gid / half;
  const int pr = int(gid % half);
  _Float16* x = rows + r * hs + 2 * pr;
  const float c = float(cossin[2 * pr]), sn = float(cossin[2 * pr + 1]);
  const float x0 = float(x[0]), x1 = float(x[1]);
  x[0] = (_Float16)(x0 * c - x1 * sn);
  x[1] = (_Float16)(x0 * sn + x1 * c);
}
// elements spanned by a strided 4-d tensor
static size_t span4(int n0, long long s0, int n1, long long s1, int n2, long long s2, int n3, long long s3) {
  return size_t((n0 - 1) * s0 + (n1 - 1) * s1 + (n2 - 1) * s2 + (n3 - 1) * s3 + 1);
}
// set_error(error) (unless empty: the error is already set) and the line the reference's callers look for on stderr
static void attn_fail(const std::string& error, const std::string& shown) {
  if (!error.empty()) set_error(error);
  fprintf(stderr, "Err: invalid parameters (%s)\n", shown.c_str());
}

}  // namespace ns

using namespace ns;  // NOLINT

extern "C" {

void bestla_reordered_attn_fp32_batch_kv_info(const kv_shape_t* params, kv_cache_info_t* out) {
  // mha_dense.cpp:82-112.  Byte strides, as the graph code uses them for its views (llama.cpp:544-560)
  if (!params || !out) return;
  const size_t row = size_t(params->head_size) * 2;
  out->k_layout = ATTN_FWD_LAYOUT_PLAIN;
  out->v_layout = ATTN_FWD_LAYOUT_PLAIN;
  out->stride_k_head_size = 2;
  out->stride_k_sl = int(row);
  out->stride_k_head_num = int(row * params->sl_kv_max);
  out->k_bytes = size_t(out->stride_k_head_num) * params->heads_kv;
  out->stride_v_head_size = 2;
  out->stride_v_sl = int(row);
  out->stride_v_head_num = int(row * params->sl_kv_max);
  out->v_bytes = size_t(out->stride_v_head_num) * params->heads_kv;
}

// ---- device mirrors of the library-managed kv caches -----------------------------------------------------------------------
// The graph keeps a library-managed cache (NE_TYPE_BTLA tensors, llama.cpp:544-560) in HOST memory and hands its address to every
// entry below; nothing but these entries ever reads or writes its bytes (the layout is this library's own).  Uploading the
// visible K / V rows for every attention call (32 MB per layer and token at 2048 positions) made the default, host-pointer
// route PCIe-bound.  So every cache the update entries see gets a DEVICE MIRROR, keyed by its host address range: updates,
// shifts and beam copies are applied to both copies (the host copy stays authoritative and complete), the attention entry
// reads the mirror.  A range that is not (wholly) mirrored falls back to the upload path; a new range that overlaps an old
// one replaces it (the tensor was re-created); ns_hip_cache_clear() and NS_KV_MIRROR=0 drop / disable the mirrors — needed
// only by a caller that writes cache bytes behind the library's back (restoring a saved session with memcpy).
static std::mutex g_attn_host_mu;  // the mirrors, and the host-tensor entries' staging slots in the null stream's scratch: one call at a time
struct KvMirror {
  char* dev = nullptr;
  size_t bytes = 0;
};
static std::map<const char*, KvMirror> g_kv_mirrors;  // host base -> mirror; guarded by g_attn_host_mu
static bool kv_mirror_enabled() {
  static const bool on = !(getenv("NS_KV_MIRROR") && atoi(getenv("NS_KV_MIRROR")) == 0);
  return on;
}
// device address of host range [p, p + bytes) when a mirror covers it, else nullptr
static char* kv_mirror_find(const char* p, size_t bytes) {
  auto it = g_kv_mirrors.upper_bound(p);
  if (it == g_kv_mirrors.begin()) return nullptr;
  --it;
  if (p >= it->first && p + bytes <= it->first + it->second.bytes) return it->second.dev + (p - it->first);
  return nullptr;
}
// mirror of exactly [p, p + bytes): the covering one, or a new one filled from the host copy (overlapping older ones go)
static char* kv_mirror_get(const char* p, size_t bytes) {
  if (!kv_mirror_enabled() || bytes == 0) return nullptr;
  if (char* d = kv_mirror_find(p, bytes)) return d;
  for (auto it = g_kv_mirrors.begin(); it != g_kv_mirrors.end();) {
    if (it->first < p + bytes && p < it->first + it->second.bytes) {
      (void)hipFree(it->second.dev);
      it = g_kv_mirrors.erase(it);
    } else {
      ++it;
    }
  }
  KvMirror m;
  if (hipMalloc(reinterpret_cast<void**>(&m.dev), bytes) != hipSuccess || hipMemcpy(m.dev, p, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    if (m.dev) (void)hipFree(m.dev);
    return nullptr;  // no mirror: the upload path serves this cache
  }
  m.bytes = bytes;
  g_kv_mirrors[p] = m;
  return m.dev;
}

// pinned, device-mapped staging for the decode-sized host calls (guarded by g_attn_host_mu): the kernels read / write host
// memory over PCIe, a call is memcpy + launches + ONE synchronisation instead of blocking hipMemcpy round trips
struct AttnPinned {
  void* host = nullptr;
  void* dev = nullptr;
  size_t cap = 0;
};
static AttnPinned g_attn_pin[4];
constexpr size_t kAttnZeroCopyMax = size_t(2) << 20;
static bool attn_zero_copy() {
  static const bool off = getenv("NS_NO_ZERO_COPY") != nullptr;  // diagnostics
  return !off;
}
static void* attn_pinned(int slot, size_t bytes, void** dev) {
  AttnPinned& e = g_attn_pin[slot];
  if (bytes > e.cap) {
    if (e.host) (void)hipHostFree(e.host);
    e = AttnPinned{};
    const size_t want = bytes < (size_t(1) << 16) ? (size_t(1) << 16) : bytes;
    if (hipHostMalloc(&e.host, want, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&e.dev, e.host, 0) != hipSuccess) {
      (void)hipGetLastError();
      if (e.host) (void)hipHostFree(e.host);
      e = AttnPinned{};
      return nullptr;
    }
    e.cap = want;
  }
  *dev = e.dev;
  return e.host;
}
static bool kv_device() { return attn_device_visible("bestla_reordered_attn"); }

// update_k / update_v share one layout here: fp32 rows (any element steps) -> fp16 at [batch][head][seq_off + i][:]
static void kv_update(const bestla_fusion_attn_fp32_update_kv_args_t* pp, const char* who) {
  ns::HostScope host_scope("bestla_reordered_attn_fp32_update_k/v");
  if (!kv_device()) return;
  const auto& a = *pp;
  if (!a.src || !a.cache || a.batch_size < 0 || a.heads_kv <= 0 || a.head_size <= 0 || a.seq_size < 0 || a.seq_off < 0 ||
      a.seq_off + a.seq_size > a.seq_max)
    return attn_fail(std::string(who) + ": invalid argument", who);
  const size_t total = size_t(a.batch_size) * a.heads_kv * a.seq_size * a.head_size;
  if (total == 0) return;
  // src -> out [batch][head][seq][hs] (+ the rows of the cache's device mirror), on the null stream
  auto launch = [&](const float* src, _Float16* out, _Float16* mirror) {
    hipLaunchKernelGGL(kv_update_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, nullptr, src, out, a.batch_size, a.heads_kv, a.head_size,
                       a.seq_size, (long long)a.step_bs, (long long)a.step_head_num, (long long)a.step_seq, (long long)a.step_head_size, mirror,
                       a.seq_max, a.seq_off);
    return hipGetLastError() == hipSuccess;
  };
  const size_t nsrc = span4(a.batch_size, a.step_bs, a.heads_kv, a.step_head_num, a.seq_size, a.step_seq, a.head_size, a.step_head_size);
  std::lock_guard<std::mutex> host_lock(g_attn_host_mu);
  const size_t row_b = size_t(a.head_size) * 2;
  if (attn_zero_copy() && nsrc * 4 + total * 2 <= kAttnZeroCopyMax) {  // a token's rows: pinned staging, one launch, one synchronisation
    void *zsrc = nullptr, *zout = nullptr;
    float* hsrc = static_cast<float*>(attn_pinned(0, nsrc * 4, &zsrc));
    _Float16* hout = static_cast<_Float16*>(attn_pinned(1, total * 2, &zout));
    if (hsrc && hout) {
      const size_t slab = size_t(a.batch_size) * a.heads_kv * a.seq_max * row_b;
      const bool had = kv_mirror_find(a.cache, slab) != nullptr;  // (a mirror created now is filled from the host copy below)
      _Float16* mir = had ? reinterpret_cast<_Float16*>(kv_mirror_find(a.cache, slab)) : nullptr;
      memcpy(hsrc, a.src, nsrc * 4);
      if (launch(static_cast<const float*>(zsrc), static_cast<_Float16*>(zout), mir) && hipStreamSynchronize(nullptr) == hipSuccess) {
        const size_t chunk = size_t(a.seq_size) * row_b;
        for (size_t bh = 0; bh < size_t(a.batch_size) * a.heads_kv; bh++)
          memcpy(a.cache + (bh * a.seq_max + a.seq_off) * row_b, reinterpret_cast<const char*>(hout) + bh * chunk, chunk);
        if (!had) (void)kv_mirror_get(a.cache, slab);  // first sight of this cache: mirror = the (now complete) host copy
      } else {
        (void)hipGetLastError();
        attn_fail(std::string(who) + ": device launch failed", std::string(who) + ": device launch failed");
      }
      return;
    }
  }
  // staging in the grow-only per-stream scratch (a hipMalloc / hipFree pair per call synchronises the whole device twice)
  float* dsrc = static_cast<float*>(stream_scratch(nullptr, nsrc * 4, SLOT_KV_HOST_A));
  _Float16* dout = static_cast<_Float16*>(stream_scratch(nullptr, total * 2, SLOT_KV_HOST_B));
  bool ok = dsrc && dout && hipMemcpy(dsrc, a.src, nsrc * 4, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    // [batch x head] chunks of seq_size rows land at row seq_off of their seq_max-row slab
    const size_t row = size_t(a.head_size) * 2;
    ok = launch(dsrc, dout, nullptr) &&
         hipMemcpy2D(a.cache + size_t(a.seq_off) * row, size_t(a.seq_max) * row, dout, size_t(a.seq_size) * row,
                     size_t(a.seq_size) * row, size_t(a.batch_size) * a.heads_kv, hipMemcpyDeviceToHost) == hipSuccess;
    // the device mirror of this cache (created from the host copy — which the line above just completed — on first sight)
    if (ok) {
      const size_t slab = size_t(a.batch_size) * a.heads_kv * a.seq_max * row;
      const bool fresh = kv_mirror_find(a.cache, slab) == nullptr;
      char* mir = kv_mirror_get(a.cache, slab);
      if (mir && !fresh)
        ok = hipMemcpy2D(mir + size_t(a.seq_off) * row, size_t(a.seq_max) * row, dout, size_t(a.seq_size) * row, size_t(a.seq_size) * row,
                         size_t(a.batch_size) * a.heads_kv, hipMemcpyDeviceToDevice) == hipSuccess;
    }
  }
  if (!ok) {
    (void)hipGetLastError();
    attn_fail(std::string(who) + ": device copy / launch failed", std::string(who) + ": device copy / launch failed");
  }
}
void bestla_reordered_attn_fp32_update_k(const bestla_fusion_attn_fp32_update_kv_args_t* params) {
  kv_update(params, "bestla_reordered_attn_fp32_update_k");
}
void bestla_reordered_attn_fp32_update_v(const bestla_fusion_attn_fp32_update_kv_args_t* params) {
  kv_update(params, "bestla_reordered_attn_fp32_update_v");
}

void bestla_reordered_attn_fp32_shift_rope_k(char* cache, const uint16_t* cossin, int batch_size, int heads_kv, int head_size,
                                             int seq_max, int seq_keep) {
  if (!kv_device()) return;
  if (!cache || !cossin || batch_size < 0 || heads_kv <= 0 || head_size <= 0 || (head_size & 1) || seq_keep < 0 || seq_keep > seq_max)
    return attn_fail("bestla_reordered_attn_fp32_shift_rope_k: invalid argument", "bestla_reordered_attn_fp32_shift_rope_k");
  const size_t row = size_t(head_size) * 2, slabs = size_t(batch_size) * heads_kv, n = size_t(seq_max - seq_keep);
  if (slabs == 0 || n == 0) return;
  std::lock_guard<std::mutex> host_lock(g_attn_host_mu);
  _Float16* drows = static_cast<_Float16*>(stream_scratch(nullptr, slabs * n * row, SLOT_KV_HOST_A));
  _Float16* dcs = static_cast<_Float16*>(stream_scratch(nullptr, row, SLOT_KV_HOST_B));
  bool ok = drows && dcs && hipMemcpy(dcs, cossin, row, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy2D(drows, n * row, cache + size_t(seq_keep) * row, size_t(seq_max) * row, n * row, slabs, hipMemcpyHostToDevice) ==
                hipSuccess;
  if (ok) {
    const size_t work = slabs * n * (head_size / 2);
    hipLaunchKernelGGL(kv_shift_rope_kernel, dim3(unsigned((work + 255) / 256)), dim3(256), 0, nullptr, drows, dcs, slabs * n, head_size);
    ok = hipGetLastError() == hipSuccess &&
         hipMemcpy2D(cache + size_t(seq_keep) * row, size_t(seq_max) * row, drows, n * row, n * row, slabs, hipMemcpyDeviceToHost) ==
             hipSuccess;
    if (ok)
      if (char* mir = kv_mirror_find(cache, slabs * size_t(seq_max) * row))
        ok = hipMemcpy2D(mir + size_t(seq_keep) * row, size_t(seq_max) * row, drows, n * row, n * row, slabs, hipMemcpyDeviceToDevice) ==
             hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    const char* text = "bestla_reordered_attn_fp32_shift_rope_k: device copy / launch failed";
    attn_fail(text, text);
  }
}

// beam search: rows [seq_off, seq_off + seq_size) of every head from one sequence's cache to another's (both in host
// memory, as the graph allocates them): a plain copy in this layout — data movement, no arithmetic
static void kv_batch_cpy(const bestla_fusion_attn_fp32_batch_cpy_kv_args_t* pp) {
  ns::HostScope host_scope("bestla_fusion_attn_fp32_batch_cpy_k/v");
  const auto& a = *pp;
  if (!a.src || !a.dst || a.heads_kv <= 0 || a.head_size <= 0 || a.seq_size <= 0 || a.seq_off < 0 || a.seq_off + a.seq_size > a.seq_max) return;
  const size_t row = size_t(a.head_size) * 2;
  for (int h = 0; h < a.heads_kv; h++)
    memcpy(a.dst + (size_t(h) * a.seq_max + a.seq_off) * row, a.src + (size_t(h) * a.seq_max + a.seq_off) * row, size_t(a.seq_size) * row);
  // the destination's device mirror takes the same rows (from the host copy just written: a beam copy is a few rows)
  std::lock_guard<std::mutex> host_lock(g_attn_host_mu);
  const size_t slab = size_t(a.heads_kv) * a.seq_max * row;
  if (char* mir = kv_mirror_find(a.dst, slab)) {
    if (hipMemcpy2D(mir + size_t(a.seq_off) * row, size_t(a.seq_max) * row, a.dst + size_t(a.seq_off) * row, size_t(a.seq_max) * row,
                    size_t(a.seq_size) * row, size_t(a.heads_kv), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      for (auto it = g_kv_mirrors.begin(); it != g_kv_mirrors.end(); ++it)  // cannot keep it current: drop it, the upload path takes over
        if (a.dst >= it->first && a.dst < it->first + it->second.bytes) {
          (void)hipFree(it->second.dev);
          g_kv_mirrors.erase(it);
          break;
        }
    }
  }
}
void bestla_fusion_attn_fp32_batch_cpy_k(const bestla_fusion_attn_fp32_batch_cpy_kv_args_t* params) { kv_batch_cpy(params); }
void bestla_fusion_attn_fp32_batch_cpy_v(const bestla_fusion_attn_fp32_batch_cpy_kv_args_t* params) { kv_batch_cpy(params); }

void bestla_reordered_attn_fp32_forward(const bestla_reordered_attn_fp32_fp32_fwd_args_t* rp) {
  ns::HostScope host_scope("bestla_reordered_attn_fp32_forward");
  // the graph passes BYTE strides of its K / V views (ne_layers.c:10238-10279; the sequence stride of V is not passed at
  // all: every layout knows its own) — here they are plain fp16 rows, so this is the fp16 attention entry
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = rp->Q, a.K = reinterpret_cast<uint16_t*>(rp->K), a.V = reinterpret_cast<uint16_t*>(rp->V), a.dst = rp->dst;
  a.Q_sc = rp->Q_sc, a.K_sc = rp->K_sc, a.V_sc = rp->V_sc, a.dst_sc = rp->dst_sc;
  a.tmp = rp->tmp, a.QK_scale = rp->QK_scale, a.attn_flags = rp->attn_flags;
  a.batch_size = rp->batch_size, a.head_num = rp->head_num, a.heads_kv = rp->heads_kv, a.head_size = rp->head_size;
  a.sl_q = rp->sl_q, a.sl_kv = rp->sl_kv;
  a.Q_layout = a.K_layout = a.V_layout = a.dst_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.step_q_bs = rp->step_q_bs, a.step_q_head_num = rp->step_q_head_num, a.step_q_sl = rp->step_q_sl;
  a.step_k_bs = rp->stride_k_bs / 2, a.step_k_head_num = rp->stride_k_head_num / 2;
  a.step_k_sl = rp->stride_k_sl ? rp->stride_k_sl / 2 : rp->head_size, a.step_k_head_size = 1;
  a.step_v_bs = rp->stride_v_bs / 2, a.step_v_head_num = rp->stride_v_head_num / 2, a.step_v_sl = rp->head_size, a.step_v_head_size = 1;
  a.step_dst_bs = rp->step_dst_bs, a.step_dst_head_num = rp->step_dst_head_num, a.step_dst_sl = rp->step_dst_sl;
  if (rp->K_layout != ATTN_FWD_LAYOUT_PLAIN || rp->V_layout != ATTN_FWD_LAYOUT_PLAIN)
    return attn_fail("bestla_reordered_attn_fp32_forward: the cache was not laid out by this library (bestla_reordered_attn_fp32_batch_kv_info)",
                     "bestla_reordered_attn_fp32_forward: foreign cache layout");
  bestla_fusion_attn_fp32_fp16_fp16_fp32_forward(&a);
}

void bestla_fusion_attn_fp32_fp16_fp16_fp32_forward(const attn_fp32_fp16_fp16_fp32_fwd_args_t* hp) {
  // host tensors (reference semantics): upload the spans the strides describe, run, download dst, synchronous
  const std::string who = "bestla_fusion_attn_fp32_fp16_fp16_fp32_forward: ";
  if (!attn_device_visible("bestla_fusion_attn_fp32_fp16_fp16_fp32_forward")) return;
  attn_fp32_fp16_fp16_fp32_fwd_args_t a = *hp;
  const size_t nq = span4(a.batch_size, a.step_q_bs, a.head_num, a.step_q_head_num, a.sl_q, a.step_q_sl, a.head_size, 1);
  const size_t nk = span4(a.batch_size, a.step_k_bs, a.heads_kv, a.step_k_head_num, a.sl_kv, a.step_k_sl, a.head_size,
                          a.step_k_head_size);
  const size_t nv = span4(a.batch_size, a.step_v_bs, a.heads_kv, a.step_v_head_num, a.sl_kv, a.step_v_sl, a.head_size,
                          a.step_v_head_size);
  const size_t nd = span4(a.batch_size, a.step_dst_bs, a.head_num, a.step_dst_head_num, a.sl_q, a.step_dst_sl,
                          a.head_size, 1);
  // staging in the grow-only per-stream scratch (four hipMalloc / hipFree pairs per call synchronised the device eight times)
  std::lock_guard<std::mutex> host_lock(g_attn_host_mu);
  // K / V of a library-managed cache are already on the device (kv mirrors above): nothing to upload
  void* mk = kv_mirror_find(reinterpret_cast<const char*>(hp->K), nk * 2);
  void* mv = kv_mirror_find(reinterpret_cast<const char*>(hp->V), nv * 2);
  if (mk && mv && attn_zero_copy() && (nq + nd) * 4 <= kAttnZeroCopyMax) {  // decode over a mirrored cache: Q and dst through pinned memory
    void *zq = nullptr, *zd = nullptr;
    float* hq = static_cast<float*>(attn_pinned(2, nq * 4, &zq));
    float* hd = static_cast<float*>(attn_pinned(3, nd * 4, &zd));
    if (hq && hd) {
      memcpy(hq, hp->Q, nq * 4);
      memcpy(hd, hp->dst, nd * 4);  // keeps the bytes between strided rows
      a.Q = static_cast<float*>(zq);
      a.K = static_cast<uint16_t*>(mk);
      a.V = static_cast<uint16_t*>(mv);
      a.dst = static_cast<float*>(zd);
      a.tmp = nullptr;
      const bool okz = ns_hip_attn_fp32_fp16_fp16_fp32_forward(&a, nullptr) == 0 && hipStreamSynchronize(nullptr) == hipSuccess;
      if (okz) memcpy(hp->dst, hd, nd * 4);
      else attn_fail("", who + ns_hip_last_error());
      return;
    }
  }
  void* dq = stream_scratch(nullptr, nq * 4, SLOT_KV_HOST_A);
  void* dk = mk ? mk : stream_scratch(nullptr, nk * 2, SLOT_KV_HOST_B);
  void* dv = mv ? mv : stream_scratch(nullptr, nv * 2, SLOT_KV_HOST_C);
  void* dd = stream_scratch(nullptr, nd * 4, SLOT_KV_HOST_D);
  bool ok = dq && dk && dv && dd;
  ok = ok && hipMemcpy(dq, hp->Q, nq * 4, hipMemcpyHostToDevice) == hipSuccess &&
       (mk || hipMemcpy(dk, hp->K, nk * 2, hipMemcpyHostToDevice) == hipSuccess) &&
       (mv || hipMemcpy(dv, hp->V, nv * 2, hipMemcpyHostToDevice) == hipSuccess) &&
       hipMemcpy(dd, hp->dst, nd * 4, hipMemcpyHostToDevice) == hipSuccess;  // keeps bytes between strided rows
  if (ok) {
    a.Q = static_cast<float*>(dq);
    a.K = static_cast<uint16_t*>(dk);
    a.V = static_cast<uint16_t*>(dv);
    a.dst = static_cast<float*>(dd);
    a.tmp = nullptr;  // the caller's tmp is host memory: partials go to the internal device scratch
    ok = ns_hip_attn_fp32_fp16_fp16_fp32_forward(&a, nullptr) == 0 && hipDeviceSynchronize() == hipSuccess &&
         hipMemcpy(hp->dst, dd, nd * 4, hipMemcpyDeviceToHost) == hipSuccess;
  } else {
    set_error("attention: device allocation / upload failed");
  }
  if (!ok) attn_fail("", who + ns_hip_last_error());
}

}  // extern "C"

namespace ns {
void kv_mirrors_clear() {
  std::lock_guard<std::mutex> lock(g_attn_host_mu);
  for (auto& kv : g_kv_mirrors) (void)hipFree(kv.second.dev);
  g_kv_mirrors.clear();
}
void touch_kvcache_module() { touch_kernel(reinterpret_cast<const void*>(kv_update_kernel)); }
}  // namespace ns
