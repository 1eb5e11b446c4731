// ns_api.cpp — C ABI of libns_hip.so (declared in include/ns_bestla.h): what every part of it stands on — the error string, the device
// check, the tuning switches, warm-up — and the thin device-pointer wrappers (norm, RoPE, silu, dup, mul, add, quantize).  The rest of
// the surface: ns_weights.cpp (blob -> device weight), ns_dispatch.cpp (forwards and fused entries), ns_host_entry.cpp (host pointers).
//
// Mirrors the reference's operator boundary:
//   neural_speed/core/ne_bestla.h:21-83, :99-109             (extern "C" surface; the device twins of its element-wise operators)
// There is no CPU compute fallback anywhere behind this surface: without a HIP device every compute entry reports an error.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "ns_api_int.h"
#include "ns_attn.h"
#include "ns_route.h"
#include "ns_route_op.h"

using namespace ns;  // NOLINT

namespace {
// Per calling thread, like errno: a failure on one thread is never reported to (or overwritten by) another.
thread_local std::string g_err;
}  // namespace
namespace ns {
bool hip_ok(hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return false;
}

bool launched(hipError_t e, const char* what, int* rc) {
  if (e == hipErrorNotSupported) return false;
  *rc = hip_ok(e, what) ? 0 : -1;
  return true;
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

void set_error(const std::string& s) { g_err = s; }

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

namespace {
// ns_hip_set_tuning's keys and what each one sets
struct TuningKey {
  const char* key;
  void (*set)(int);
};
const TuningKey kTuning[] = {
    {"gemv2", set_gemv_mode},
    {"gvs", [](int v) { set_gemvs_tuning(0, v); }},
    {"gvs_slices", [](int v) { set_gemvs_tuning(1, v); }},
    {"gvs_waves", [](int v) { set_gemvs_tuning(2, v); }},
    {"gvs_grid", [](int v) { set_gemvs_tuning(3, v); }},
    {"gvs_table", [](int v) { set_gemvs_tuning(4, v); }},
    {"gvs_finalize", [](int v) { set_gemvs_tuning(5, v); }},
    // row thresholds of ns_hip_mul_mat_id's paths; 0 = default, < 0 = off
    {"moe_gemv_rows", [](int v) { set_moe_tuning(0, v); }},
    {"moe_grouped_rows", [](int v) { set_moe_tuning(1, v); }},
    {"moe_ffn_grouped_rows", set_moe_ffn_grouped_rows},  // ns_hip_moe_ffn_silu / _gelu: rows from which the grouped pass serves a call (0 = default, < 0 = never)
    {"moe_ffn_device_rows", set_moe_ffn_device_rows},  // ns_hip_moe_ffn_silu / _gelu: rows up to which the device-grouped pass serves a call (0 = default: never)
    {"moe_ffn_chunk_rows", set_moe_ffn_chunk_rows},    // ... a cap of 1 .. 16 on the rows of its chunks (0 = by LDS fit)
    {"moe_ffn_fused", set_moe_ffn_fused},  // ns_hip_moe_ffn_silu / _gelu: 0 = always the composition, 1 / -1 = the fused launches inside their envelope
    {"g3_min_m", set_gemm3_min_m},
    {"i8_tile", set_i8_tile},
    {"i8_mfma", set_i8_mfma_gen},
    {"attn_heads_first", set_attn_heads_first},
    {"g3_wide", set_gemm3_wide},
    {"g3_f8", set_gemm3_f8},  // fp8 weights on the tiled prefill GEMM (1, default) or as before it took them (0); -1: NS_G3_F8 / default
    {"g3_bm", set_gemm3_bm},
    {"gv_nw", set_decode_waves},  // (value checked by ns_hip_set_tuning)
    {"gv_rows1", set_gemv_rows1},
    {"attn_wg_target", [](int v) { set_attn_tuning(v, 0); }},
    {"attn_min_keys", [](int v) { set_attn_tuning(0, v); }},
    {"planes", set_gemv_planes},
    {"planes_load", set_planes_load},
    {"attn_mfma2_rows", set_attn_mfma2_rows},
    {"attn_stream_wg_target", [](int v) { set_attn_stream_tuning(v, 0); }},
    {"attn_stream_min_keys", [](int v) { set_attn_stream_tuning(0, v); }},
    {"attn_stream", set_attn_stream},
    {"attn_inlaunch", set_attn_inlaunch},
    {"attn_block_split", set_attn_block_split},  // (opt-in: 0 = off, the default)
    {"attn_block_wg_target", [](int v) { set_attn_block_tuning(v, 0); }},
    {"attn_block_min_keys", [](int v) { set_attn_block_tuning(0, v); }},
    // the device route's attention reads the fp16 mirror of the fp32 kv cache (1, default) or the fp32 cache itself (0); -1: NS_DEVICE_KV
    {"device_kv_f16", kv16_set},
};
}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------------ part 3
void ns_hip_reset_error(void) {
  // drops a sticky HIP error (e.g. after a stream capture was invalidated) and the library's error string
  for (int i = 0; i < 8 && hipGetLastError() != hipSuccess; i++) {
  }
  set_error("");
}

int ns_hip_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

const char* ns_hip_last_error(void) { return g_err.c_str(); }

int ns_hip_set_tuning(const char* key, int value) {
  for (const TuningKey& t : kTuning) {
    if (!key || strcmp(key, t.key)) continue;
    if (!strcmp(key, "gv_nw") && value != 0 && value != 2 && value != 4 && value != 8 && value != 16) {
      set_error("ns_hip_set_tuning: gv_nw must be 0, 2, 4, 8 or 16");
      return -1;
    }
    t.set(value);
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

int ns_hip_norm_prep(int m, int n, const float* dX, int ldx, const float* dGamma, void* dX16, float* dSsq, int ssq_stride,
                     void* stream) {
  if (!have_device()) return -1;
  if (!dX || m < 0 || n < 0 || ldx < n || (dSsq && ssq_stride < (n + 15) / 16)) {
    set_error("norm_prep: invalid argument");
    return -1;
  }
  return hip_ok(launch_norm_prep(m, n, dX, ldx, dGamma, dX16, dSsq, ssq_stride, (hipStream_t)stream), "norm_prep launch") ? 0 : -1;
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
      (void)moe_exp_table();  // the router's exponential table (ns_hip_moe_route): uploaded here, outside any capture
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

int ns_hip_quantize_fp_u8_colblock(int row, int col, const float* dSrc, int ld_src, uint8_t* dDst, int ld_dst,
                                   float* dScales, int ld_scale, uint8_t* dZps, int blocksize, float* dBlkReduce,
                                   void* stream) {
  if (!have_device()) return -1;
  if (!dSrc || !dDst || !dScales || !dZps || row < 0 || col < 0 || blocksize <= 0) {
    set_error("quantize_fp_u8_colblock: invalid argument");
    return -1;
  }
  if (!dBlkReduce && row >= 16) {  // GEMM-sized, no block sums wanted: the vector form (bit-identical codes, scales, zero points)
    int rc;
    if (launched(launch_aquant_u8_vec(row, col, dSrc, ld_src, dDst, ld_dst, dScales, ld_scale, dZps, blocksize, nullptr, 0, false,
                                      (hipStream_t)stream), "activation quantize launch", &rc)) return rc;
  }
  return hip_ok(launch_aquant_u8(row, col, dSrc, ld_src, dDst, ld_dst, dScales, ld_scale, dZps, blocksize, dBlkReduce,
                                 (hipStream_t)stream), "activation quantize launch") ? 0 : -1;
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
    return route_submit(route_op_rope(dSrc, dDst, batch, seq, heads, head_size, n_past, n_dims, mode, freq_base, freq_scale, ext_factor, attn_factor));
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
int ns_hip_rope_f32_yarn(const float* dSrc, float* dDst, int batch, int seq, int heads, int head_size, int n_past,
                         int n_dims, int mode, float freq_base, float freq_scale, int n_orig_ctx, float ext_factor,
                         float attn_factor, float beta_fast, float beta_slow, void* stream) {
  if (route_hook(stream)) {
    return route_submit(route_op_rope_yarn(dSrc, dDst, batch, seq, heads, head_size, n_past, n_dims, mode, freq_base, freq_scale, n_orig_ctx, ext_factor, attn_factor,
                                           beta_fast, beta_slow));
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
int ns_hip_rope_qkv_append_rows(float* dQ, const float* dK, const float* dV, void* dKcache16, void* dVcache16, int rows, int heads, int heads_kv,
                                int head_size, const int* dPos, int pos_cap, int n_dims, int mode, float freq_base, float freq_scale,
                                float ext_factor, float attn_factor, long long cache_step_bs, long long cache_step_sl, long long cache_step_head,
                                void* stream) {
  if (!have_device()) return -1;
  if (!dQ || !dK || !dV || !dKcache16 || !dVcache16 || !dPos || rows < 0 || heads <= 0 || heads_kv <= 0 || head_size <= 0 || (head_size & 1) ||
      n_dims <= 0 || (n_dims & 1) || n_dims > head_size || pos_cap < 0) {
    set_error("rope_qkv_append_rows: invalid argument");
    return -1;
  }
  if ((mode & ~2) != 0 || ext_factor != 0.f || ((mode & 2) && head_size % n_dims != 0)) {
    set_error("rope_qkv_append_rows: only modes 0 and 2 (NeoX, head_size a multiple of n_dims) without YaRN extrapolation");
    return -1;
  }
  return hip_ok(launch_rope_qkv_append_rows(dQ, dK, dV, dKcache16, dVcache16, rows, heads, heads_kv, head_size, dPos, pos_cap, n_dims, mode, freq_base,
                                            freq_scale, attn_factor, cache_step_bs, cache_step_sl, cache_step_head, (hipStream_t)stream),
                "rope/kv-append (rows) launch") ? 0 : -1;
}
// what the two writers of a paged cache ask of its description (the attention's plan states the same rules, ns_attn_plan.cpp); nullptr: in order
static const char* paged_cache_refusal(const AttnPage& pg, int heads_kv, int head_size, long long c_sl, long long c_head) {
  if (!pg.table) return "the block table is null";
  if (pg.block_shift < 0) return "block_keys must be a power of two from 16 to 256";
  if (pg.pool_blocks < 1) return "pool_blocks must be at least 1";
  if (pg.table_stride < 1) return "table_stride must be at least 1";
  if (c_sl < 0 || c_head < 0 || pg.block_step < 1 ||
      (long long)((1 << pg.block_shift) - 1) * c_sl + (long long)(heads_kv - 1) * c_head + head_size > pg.block_step)
    return "a block's keys and kv heads (cache_step_sl / cache_step_head) do not fit inside block_step";
  return nullptr;
}
int ns_hip_rope_qkv_append_paged(float* dQ, const float* dK, const float* dV, void* dKpool16, void* dVpool16, int rows, int heads, int heads_kv,
                                 int head_size, const int* dPos, int pos_cap, int n_dims, int mode, float freq_base, float freq_scale, float ext_factor,
                                 float attn_factor, const int* dBlockTable, int table_stride, int block_keys, int pool_blocks, long long block_step,
                                 long long cache_step_sl, long long cache_step_head, void* stream) {
  if (!have_device()) return -1;
  if (!dQ || !dK || !dV || !dKpool16 || !dVpool16 || !dPos || rows < 0 || heads <= 0 || heads_kv <= 0 || head_size <= 0 || (head_size & 1) ||
      n_dims <= 0 || (n_dims & 1) || n_dims > head_size || pos_cap < 0) {
    set_error("rope_qkv_append_paged: invalid argument");
    return -1;
  }
  if ((mode & ~2) != 0 || ext_factor != 0.f || ((mode & 2) && head_size % n_dims != 0)) {
    set_error("rope_qkv_append_paged: only modes 0 and 2 (NeoX, head_size a multiple of n_dims) without YaRN extrapolation");
    return -1;
  }
  const AttnPage pg = {dBlockTable, table_stride, attn_block_shift(block_keys), pool_blocks, block_step};
  if (const char* text = paged_cache_refusal(pg, heads_kv, head_size, cache_step_sl, cache_step_head)) {
    set_error(std::string("rope_qkv_append_paged: ") + text);
    return -1;
  }
  return hip_ok(launch_rope_qkv_append_paged(dQ, dK, dV, dKpool16, dVpool16, rows, heads, heads_kv, head_size, dPos, pos_cap, n_dims, mode, freq_base,
                                             freq_scale, attn_factor, pg, cache_step_sl, cache_step_head, (hipStream_t)stream),
                "rope/kv-append (paged) launch") ? 0 : -1;
}
int ns_hip_rope_qkv_append_paged_seq(float* dQ, const float* dK, const float* dV, void* dKpool16, void* dVpool16, int rows, int heads, int heads_kv,
                                     int head_size, const int* dPos, int pos_cap, int n_dims, int mode, float freq_base, float freq_scale,
                                     float ext_factor, float attn_factor, const int* dRowReq, int requests, const int* dBlockTable, int table_stride,
                                     int block_keys, int pool_blocks, long long block_step, long long cache_step_sl, long long cache_step_head,
                                     void* stream) {
  if (!have_device()) return -1;
  if (!dQ || !dK || !dV || !dKpool16 || !dVpool16 || !dPos || !dRowReq || requests < 0 || rows < 0 || heads <= 0 || heads_kv <= 0 || head_size <= 0 ||
      (head_size & 1) || n_dims <= 0 || (n_dims & 1) || n_dims > head_size || pos_cap < 0) {
    set_error("rope_qkv_append_paged_seq: invalid argument");
    return -1;
  }
  if ((mode & ~2) != 0 || ext_factor != 0.f || ((mode & 2) && head_size % n_dims != 0)) {
    set_error("rope_qkv_append_paged_seq: only modes 0 and 2 (NeoX, head_size a multiple of n_dims) without YaRN extrapolation");
    return -1;
  }
  const AttnPage pg = {dBlockTable, table_stride, attn_block_shift(block_keys), pool_blocks, block_step};
  if (const char* text = paged_cache_refusal(pg, heads_kv, head_size, cache_step_sl, cache_step_head)) {
    set_error(std::string("rope_qkv_append_paged_seq: ") + text);
    return -1;
  }
  return hip_ok(launch_rope_qkv_append_paged_seq(dQ, dK, dV, dKpool16, dVpool16, rows, heads, heads_kv, head_size, dPos, pos_cap, dRowReq, requests, n_dims,
                                                 mode, freq_base, freq_scale, attn_factor, pg, cache_step_sl, cache_step_head, (hipStream_t)stream),
                "rope/kv-append (paged, row -> request map) launch") ? 0 : -1;
}
int ns_hip_kv_paged_store(const void* dKslab16, const void* dVslab16, long long slab_step_sl, long long slab_step_head, int pos0, int n, int heads_kv,
                          int head_size, void* dKpool16, void* dVpool16, const int* dTableRow, int table_len, int block_keys, int pool_blocks,
                          long long block_step, long long cache_step_sl, long long cache_step_head, void* stream) {
  if (!have_device()) return -1;
  if (!dKslab16 || !dVslab16 || !dKpool16 || !dVpool16 || pos0 < 0 || n < 0 || heads_kv <= 0 || head_size <= 0) {
    set_error("kv_paged_store: invalid argument");
    return -1;
  }
  const AttnPage pg = {dTableRow, table_len, attn_block_shift(block_keys), pool_blocks, block_step};
  if (const char* text = paged_cache_refusal(pg, heads_kv, head_size, cache_step_sl, cache_step_head)) {
    set_error(std::string("kv_paged_store: ") + text);
    return -1;
  }
  if ((long long)pos0 + n > ((long long)table_len << pg.block_shift)) {
    set_error("kv_paged_store: rows [pos0, pos0 + n) reach behind the request's capacity (table_len * block_keys)");
    return -1;
  }
  return hip_ok(launch_kv_paged_store(dKslab16, dVslab16, slab_step_sl, slab_step_head, pos0, n, heads_kv, head_size, dKpool16, dVpool16, pg,
                                      cache_step_sl, cache_step_head, (hipStream_t)stream),
                "kv paged store launch") ? 0 : -1;
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
  if (route_hook(stream)) return route_submit(route_op_dup(dSrc, dDst, ne, src_nb, dst_nb, dst_is_f16));
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

}  // extern "C"
