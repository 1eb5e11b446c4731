// ns_attn.cpp — fused attention behind the reference's mha_dense C surface, host side: the tunables, and the launch of
// what attn_plan (ns_attn_plan.cpp) decided.  The kernels are in ns_attn_decode.hip, ns_attn_prefill.hip and ns_attn_block.hip, the library-managed kv-cache and the
// host-tensor entries in ns_kvcache.hip.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "ns_attn.h"

namespace ns {

// ---- tunables: ns_hip_set_tuning (ns_api.cpp) and the environment, read once per process ---------------------------------------------------
static int env_int(const char* name, int otherwise) { return getenv(name) ? atoi(getenv(name)) : otherwise; }
static std::atomic<int> g_attn_stream{env_int("NS_ATTN_STREAM", 1) != 0};
static std::atomic<int> g_attn_mfma2_rows{env_int("NS_ATTN_MFMA2_ROWS", 128)};
// "attn_inlaunch": measured equal (profiles/r04ab_attn_merge_in_launch.txt: split 11.8 us + merge 4.7 us against 16.5 us in one launch, whole token
// 600 vs 590 tok/s): the cost is the write-through / ticket / read-back chain across XCDs, not the kernel boundary.
static std::atomic<int> g_attn_inlaunch{env_int("NS_ATTN_INLAUNCH", 0) != 0};
static std::atomic<int> g_attn_heads_first{env_int("NS_ATTN_HEADS_FIRST", -1)};
static std::atomic<int> g_attn_wg_target{1024}, g_attn_min_keys{128}, g_attn_wg_target_s{256}, g_attn_min_keys_s{32};
static std::atomic<int> g_alibi_heads{0}, g_alibi_off{0};  // ns_hip_attn_set_head_partition
// "attn_block_split": opt-in (0) until the default dispatch, pinned by tests/test_attn_plan.py, is changed with the numbers of docs/kernels/attention.md
static std::atomic<int> g_attn_block_split{std::max(0, env_int("NS_ATTN_BLOCK_SPLIT", 0))};
static std::atomic<int> g_attn_block_target{512}, g_attn_block_min_keys{128};
static std::atomic<uint64_t> g_attn_launches[kAttnPaths];  // ns_hip_attn_stats
void set_attn_stream(int on) { g_attn_stream.store(on != 0); }
void set_attn_mfma2_rows(int rows) { g_attn_mfma2_rows.store(rows > 0 ? rows : 128); }
void set_attn_inlaunch(int on) { g_attn_inlaunch.store(on != 0); }
void set_attn_heads_first(int on) { g_attn_heads_first.store(on < 0 ? -1 : (on != 0)); }
void set_attn_tuning(int wg_target, int min_keys) {
  if (wg_target > 0) g_attn_wg_target.store(wg_target);
  if (min_keys > 0) g_attn_min_keys.store(min_keys);
}
void set_attn_stream_tuning(int wg_target, int min_keys) {
  if (wg_target > 0) g_attn_wg_target_s.store(wg_target);
  if (min_keys > 0) g_attn_min_keys_s.store(min_keys);
}
void set_attn_block_split(int keys) { g_attn_block_split.store(std::max(0, keys)); }
void set_attn_block_tuning(int wg_target, int min_keys) {
  if (wg_target > 0) g_attn_block_target.store(wg_target);
  if (min_keys > 0) g_attn_block_min_keys.store(min_keys);
}
static AttnKnobs attn_knobs() {
  static const AttnKnobs env = [] {  // the switches only the environment sets (diagnostics, A/B runs)
    AttnKnobs k;
    k.no_mfma = getenv("NS_ATTN_NO_MFMA") != nullptr;
    k.pipe = env_int("NS_ATTN_PIPE", 1);
    k.pvar = env_int("NS_ATTN_PVAR", -1);
    k.no_xcd_map = getenv("NS_ATTN_NO_XCD_MAP") != nullptr;
    k.v1 = getenv("NS_ATTN_V1") != nullptr;
    k.dyn_ranges = env_int("NS_ATTN_DYN_RANGES", 1) != 0;
    return k;
  }();
  AttnKnobs k = env;
  k.attn_stream = g_attn_stream.load(std::memory_order_relaxed);
  k.attn_mfma2_rows = g_attn_mfma2_rows.load(std::memory_order_relaxed);
  k.attn_inlaunch = g_attn_inlaunch.load(std::memory_order_relaxed);
  k.attn_heads_first = g_attn_heads_first.load();
  k.wg_target = g_attn_wg_target.load(), k.min_keys = g_attn_min_keys.load();
  k.wg_target_s = g_attn_wg_target_s.load(), k.min_keys_s = g_attn_min_keys_s.load();
  k.alibi_heads = g_alibi_heads.load(), k.alibi_off = g_alibi_off.load();
  k.block_split = g_attn_block_split.load(std::memory_order_relaxed);
  k.block_target = g_attn_block_target.load(), k.block_min_keys = g_attn_block_min_keys.load();
  return k;
}

// scratch of a one-row plan, then its launch; *merged: attn_merge_kernel followed
static hipError_t launch_onerow_plan(AttnPlan pl, const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, AttnKnobs kn, const Affine& aff, hipStream_t st,
                                     std::string* why, bool device_tmp, void* dst16, bool* merged, const AttnPage* page = nullptr) {
  float* ws = nullptr;
  if (pl.partial_bytes) {
    // partials go to the caller's workspace (`tmp`, sized by bestla_fusion_attn_workspace_size: the reference's own contract, and the only choice
    // that works on a stream being captured for the first time); without one, to a grow-only per-stream scratch
    ws = device_tmp ? reinterpret_cast<float*>(a.tmp) : nullptr;
    if (!ws) ws = static_cast<float*>(stream_scratch(st, pl.partial_bytes, SLOT_ATTN_PARTIALS));
    if (!ws) {  // scratch allocation failed: planned again as one range, still correct
      kn.no_partials = true;
      pl = attn_plan(a, dst16, kn, aff, why, page);
    }
  }
  // (nullptr, e.g. first use on a capturing stream: the merge launch)
  uint32_t* tickets = pl.want_tickets ? static_cast<uint32_t*>(stream_scratch_zeroed(st, kAttnTicketCap * 4, SLOT_ATTN_TICKETS)) : nullptr;
  if (merged) *merged = pl.sp.nsplit > 1 && !tickets;
  return launch_attn_onerow(pl, ws, tickets, st);
}

// plan, take scratch, launch
static hipError_t launch_attn(const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, hipStream_t st, std::string* why, bool device_tmp, void* dst16) {
  AttnKnobs kn = attn_knobs();
  AttnPlan pl = attn_plan(a, dst16, kn, g_affine, why);
  float* ws = nullptr;  // (of the block-split path)
  if (pl.path == AP_BLOCK_SPLIT) {
    // bestla_fusion_attn_workspace_size does not know this path (the reference's contract, sized by the one-row rules): the caller's `tmp` serves
    // only where it is large enough, the stream's scratch otherwise; without either the call is planned as with the key at 0
    if (device_tmp && pl.partial_bytes <= attn_ws_bytes(kn, a.batch_size, a.head_num, a.heads_kv, a.head_size, a.sl_q, a.sl_kv))
      ws = reinterpret_cast<float*>(a.tmp);
    if (!ws) ws = static_cast<float*>(stream_scratch(st, pl.partial_bytes, SLOT_ATTN_PARTIALS));
    if (!ws) {
      kn.block_split = 0;
      pl = attn_plan(a, dst16, kn, g_affine, why);
    }
  }
  if (pl.path == AP_REFUSED) return hipErrorInvalidValue;
  auto counted = [&](hipError_t e) {
    if (e == hipSuccess) g_attn_launches[pl.path].fetch_add(1, std::memory_order_relaxed);
    return e;
  };
  if (pl.path == AP_BLOCK_SPLIT) return counted(launch_attn_block_split(pl, ws, st));
  if (pl.path == AP_ROWS64 || pl.path == AP_ROWS128 || pl.path == AP_PIPELINED) return counted(launch_attn_rows(pl, st));
  return counted(launch_onerow_plan(pl, a, kn, g_affine, st, why, device_tmp, dst16, nullptr));
}

// ns_hip_attn_decode_rows: the moving-length plan of the capacity, its live length read per batch entry.  The Affine is this call's own (the
// thread-local g_affine belongs to the replayed route); the merge follows the "attn_inlaunch" key as in the uniform entry.
static std::atomic<uint64_t> g_attn_rows[4];  // ns_hip_attn_rows_stats
static hipError_t launch_attn_decode_rows(const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, const int* lens, int bias, hipStream_t st, std::string* why,
                                          void* dst16) {
  if (a.sl_q != 1) {
    *why = "attention, per-request context lengths: one query row per request (sl_q must be 1)";
    return hipErrorInvalidValue;
  }
  if (!lens) {
    *why = "attention, per-request context lengths: dKvLens is null";
    return hipErrorInvalidValue;
  }
  if (a.sl_kv < 1) {
    *why = "attention, per-request context lengths: sl_kv is the capacity of a request's slab (at least 1 key)";
    return hipErrorInvalidValue;
  }
  const AttnKnobs kn = attn_knobs();
  Affine aff;
  aff.k = lens, aff.delta = 1, aff.cap = a.sl_kv, aff.inlaunch = 0, aff.rows = 1, aff.bias = bias;
  const AttnPlan pl = attn_plan(a, dst16, kn, aff, why);
  if (pl.path != AP_RING && pl.path != AP_SPLIT_REGS) {  // (refused: the plan gives nothing else to this form)
    if (why->empty()) *why = "attention, per-request context lengths: no split kernel takes this call";
    return hipErrorInvalidValue;
  }
  bool merged = false;
  const hipError_t e = launch_onerow_plan(pl, a, kn, aff, st, why, a.tmp != nullptr, dst16, &merged);
  if (e == hipSuccess) {
    g_attn_launches[pl.path].fetch_add(1, std::memory_order_relaxed);
    g_attn_rows[pl.path == AP_RING ? 0 : 1].fetch_add(1, std::memory_order_relaxed);
    if (merged) g_attn_rows[2].fetch_add(1, std::memory_order_relaxed);
  }
  return e;
}

// ns_hip_attn_decode_paged: the per-request plan of the same shape and capacity over the pools of a paged cache (attn_plan's `page`); what differs
// from launch_attn_decode_rows is the AttnPage handed on and the counters.
static std::atomic<uint64_t> g_attn_paged[4];  // ns_hip_attn_paged_stats
static hipError_t launch_attn_decode_paged(const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, const int* lens, int bias, const AttnPage& page, hipStream_t st,
                                           std::string* why, void* dst16) {
  if (a.sl_q != 1) {
    *why = "attention, paged cache: one query row per request (sl_q must be 1)";
    return hipErrorInvalidValue;
  }
  if (!lens) {
    *why = "attention, paged cache: dKvLens is null";
    return hipErrorInvalidValue;
  }
  if (a.sl_kv < 1) {
    *why = "attention, paged cache: sl_kv is the capacity of a request (at least 1 key)";
    return hipErrorInvalidValue;
  }
  const AttnKnobs kn = attn_knobs();
  Affine aff;
  aff.k = lens, aff.delta = 1, aff.cap = a.sl_kv, aff.inlaunch = 0, aff.rows = 1, aff.bias = bias;
  const AttnPlan pl = attn_plan(a, dst16, kn, aff, why, &page);
  if (pl.path != AP_RING && pl.path != AP_SPLIT_REGS) {
    if (why->empty()) *why = "attention, paged cache: no split kernel takes this call";
    return hipErrorInvalidValue;
  }
  bool merged = false;
  const hipError_t e = launch_onerow_plan(pl, a, kn, aff, st, why, a.tmp != nullptr, dst16, &merged, &page);
  if (e == hipSuccess) {
    g_attn_launches[pl.path].fetch_add(1, std::memory_order_relaxed);
    g_attn_paged[pl.path == AP_RING ? 0 : 1].fetch_add(1, std::memory_order_relaxed);
    if (merged) g_attn_paged[2].fetch_add(1, std::memory_order_relaxed);
  }
  return e;
}

// ns_hip_attn_block_paged: plan (attn_block_paged_plan), partials in the caller's `tmp` (ns_hip_attn_block_paged_workspace_size bytes) or the stream's
// scratch, the PAGED instantiation of the block-split kernel and its merge.
static std::atomic<uint64_t> g_attn_block_paged[4];  // ns_hip_attn_block_paged_stats
static hipError_t launch_attn_block_paged_call(const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, const int* q_start, const int* lens, int bias,
                                               const AttnPage& page, hipStream_t st, std::string* why, void* dst16) {
  const AttnBlockPagedPlan pl = attn_block_paged_plan(a, dst16, attn_knobs(), page, q_start, lens, bias, why);
  if (!pl.ok) return hipErrorInvalidValue;
  float* ws = reinterpret_cast<float*>(a.tmp);
  if (!ws) ws = static_cast<float*>(stream_scratch(st, pl.partial_bytes, SLOT_ATTN_PARTIALS));
  if (!ws) {
    *why = "attention, query blocks over a paged cache: no memory for the partials (give tmp, or make one eager call before a capture)";
    return hipErrorOutOfMemory;
  }
  const hipError_t e = launch_attn_block_paged(pl, ws, st);
  if (e == hipSuccess) {
    g_attn_launches[AP_BLOCK_SPLIT].fetch_add(1, std::memory_order_relaxed);
    g_attn_block_paged[pl.hs_pad == 64 ? 0 : 1].fetch_add(1, std::memory_order_relaxed);
    g_attn_block_paged[2].fetch_add(1, std::memory_order_relaxed);
  }
  return e;
}

// ns_hip_attn_prefill_paged: plan (attn_prefill_paged_plan) and ONE launch of the 128-row kernel's PAGED instantiation: no partials, no scratch
static std::atomic<uint64_t> g_attn_prefill_paged[6];  // ns_hip_attn_prefill_paged_stats
static hipError_t launch_attn_prefill_paged_call(const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, const int* q_start, const int* lens, int bias,
                                                 const AttnPage& page, hipStream_t st, std::string* why, void* dst16) {
  const AttnPrefillPagedPlan pl = attn_prefill_paged_plan(a, dst16, attn_knobs(), page, q_start, lens, bias, why);
  if (!pl.ok) return hipErrorInvalidValue;
  const hipError_t e = launch_attn_prefill_paged(pl, st);
  if (e == hipSuccess) {
    g_attn_prefill_paged[pl.hs_pad == 64 ? 0 : (pl.hs_pad == 128 ? 1 : 2)].fetch_add(1, std::memory_order_relaxed);
    if (pl.sb) g_attn_prefill_paged[3].fetch_add(1, std::memory_order_relaxed);
    if (pl.pad) g_attn_prefill_paged[4].fetch_add(1, std::memory_order_relaxed);
  }
  return e;
}

// scratch a moving-length decode launch needs (partials for the longest context, the merge tickets): allocated BEFORE the route's capture
bool attn_prepare_moving(hipStream_t st, int batch, int heads, int heads_kv, int head_size, int cap) {
  const size_t b = attn_ws_bytes(attn_knobs(), batch, heads, heads_kv, head_size, 1, cap);
  if (b && !stream_scratch(st, b, SLOT_ATTN_PARTIALS)) return false;
  return stream_scratch_zeroed(st, kAttnTicketCap * 4, SLOT_ATTN_TICKETS) != nullptr;
}

bool attn_device_visible(const char* who) {
  int count = 0;
  if (hipGetDeviceCount(&count) == hipSuccess && count > 0) return true;
  (void)hipGetLastError();
  if (who) {
    set_error("no HIP device visible: libns_hip.so has no CPU fallback");
    fprintf(stderr, "Err: invalid parameters (%s: no HIP device visible: libns_hip.so has no CPU fallback)\n", who);
  }
  return false;
}

}  // namespace ns

using namespace ns;  // NOLINT

extern "C" {

int ns_hip_attn_set_head_partition(int global_head_num, int head_offset) {
  if (global_head_num < 0 || head_offset < 0 || (global_head_num > 0 && head_offset >= global_head_num)) {
    set_error("ns_hip_attn_set_head_partition: need 0 <= head_offset < global_head_num (or 0, 0 to clear)");
    return -1;
  }
  g_alibi_heads.store(global_head_num), g_alibi_off.store(global_head_num > 0 ? head_offset : 0);
  return 0;
}

void ns_hip_attn_stats(uint64_t out[8]) {
  static_assert(kAttnPaths == 8, "ns_hip_attn_stats: one counter per AttnPath value");
  for (int i = 0; i < kAttnPaths; i++) out[i] = g_attn_launches[i].load(std::memory_order_relaxed);
}

size_t bestla_fusion_attn_workspace_size(const attn_shape_t* s) {
  // (m, l, acc) partials of the context splits; 64 bytes minimum so that callers always get a valid pointer
  return std::max<size_t>(64, attn_ws_bytes(attn_knobs(), s->batch_size, s->head_num, s->heads_kv, s->head_size, s->sl_q, s->sl_kv));
}

bool bestla_fusion_attn_fp32_fp16_fp16_fp32_support(const attn_shape_t* s) {
  std::string why;
  return attn_device_visible(nullptr) && attn_shape_ok(s->head_num, s->heads_kv, s->head_size, s->sl_q, s->sl_kv, false, &why);
}

bool bestla_fusion_attn_fp16_support(const attn_shape_t*) { return false; }  // mha_dense.h:106: fp16 Q / dst form, not offered

bool bestla_reordered_attn_fp32_support(const attn_shape_t* params) {
  // mha_dense.cpp:70-80 answers by CPU features; here: whatever the attention kernels take (fp16 cache, ns_kvcache.hip)
  std::string why;
  return params && attn_device_visible(nullptr) &&
         attn_shape_ok(params->head_num, params->heads_kv, params->head_size, params->sl_q, params->sl_kv, false, &why);
}

int ns_hip_attn_fp32_fp16_fp16_fp32_forward(const attn_fp32_fp16_fp16_fp32_fwd_args_t* a, void* stream) {
  return ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(a, nullptr, stream);
}

int ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(const attn_fp32_fp16_fp16_fp32_fwd_args_t* a, void* dst16, void* stream) {
  std::string why;
  // device API: `tmp`, when given, is DEVICE memory of bestla_fusion_attn_workspace_size(shape) bytes
  const hipError_t e = launch_attn(*a, static_cast<hipStream_t>(stream), &why, a->tmp != nullptr, dst16);
  if (e != hipSuccess) {
    set_error(why.empty() ? std::string("attention launch: ") + hipGetErrorString(e) : why);
    return -1;
  }
  return 0;
}

int ns_hip_attn_decode_rows(const attn_fp32_fp16_fp16_fp32_fwd_args_t* a, const int* dKvLens, int kv_len_bias, void* dst16, void* stream) {
  std::string why;
  const hipError_t e = a ? launch_attn_decode_rows(*a, dKvLens, kv_len_bias, static_cast<hipStream_t>(stream), &why, dst16) : hipErrorInvalidValue;
  if (e != hipSuccess) {
    g_attn_rows[3].fetch_add(1, std::memory_order_relaxed);
    set_error(why.empty() ? std::string("attention launch (per-request context lengths): ") + (a ? hipGetErrorString(e) : "null arguments") : why);
    return -1;
  }
  return 0;
}

int ns_hip_attn_decode_paged(const attn_fp32_fp16_fp16_fp32_fwd_args_t* a, const int* dKvLens, int kv_len_bias, const int* dBlockTable, int table_stride,
                             int block_keys, int pool_blocks, long long block_step, void* dst16, void* stream) {
  std::string why;
  const AttnPage page = {dBlockTable, table_stride, attn_block_shift(block_keys), pool_blocks, block_step};
  const hipError_t e = a ? launch_attn_decode_paged(*a, dKvLens, kv_len_bias, page, static_cast<hipStream_t>(stream), &why, dst16) : hipErrorInvalidValue;
  if (e != hipSuccess) {
    g_attn_paged[3].fetch_add(1, std::memory_order_relaxed);
    set_error(why.empty() ? std::string("attention launch (paged cache): ") + (a ? hipGetErrorString(e) : "null arguments") : why);
    return -1;
  }
  return 0;
}

int ns_hip_attn_block_paged(const attn_fp32_fp16_fp16_fp32_fwd_args_t* a, const int* dQStart, const int* dKvLens, int kv_len_bias, const int* dBlockTable,
                            int table_stride, int block_keys, int pool_blocks, long long block_step, void* dst16, void* stream) {
  std::string why;
  const AttnPage page = {dBlockTable, table_stride, attn_block_shift(block_keys), pool_blocks, block_step};
  const hipError_t e =
      a ? launch_attn_block_paged_call(*a, dQStart, dKvLens, kv_len_bias, page, static_cast<hipStream_t>(stream), &why, dst16) : hipErrorInvalidValue;
  if (e != hipSuccess) {
    g_attn_block_paged[3].fetch_add(1, std::memory_order_relaxed);
    set_error(why.empty() ? std::string("attention launch (query blocks over a paged cache): ") + (a ? hipGetErrorString(e) : "null arguments") : why);
    return -1;
  }
  return 0;
}

int ns_hip_attn_prefill_paged(const attn_fp32_fp16_fp16_fp32_fwd_args_t* a, const int* dQStart, const int* dKvLens, int kv_len_bias, const int* dBlockTable,
                              int table_stride, int block_keys, int pool_blocks, long long block_step, void* dst16, void* stream) {
  std::string why;
  const AttnPage page = {dBlockTable, table_stride, attn_block_shift(block_keys), pool_blocks, block_step};
  const hipError_t e =
      a ? launch_attn_prefill_paged_call(*a, dQStart, dKvLens, kv_len_bias, page, static_cast<hipStream_t>(stream), &why, dst16) : hipErrorInvalidValue;
  if (e != hipSuccess) {
    g_attn_prefill_paged[5].fetch_add(1, std::memory_order_relaxed);
    set_error(why.empty() ? std::string("attention launch (prompt blocks over a paged cache): ") + (a ? hipGetErrorString(e) : "null arguments") : why);
    return -1;
  }
  return 0;
}

void ns_hip_attn_prefill_paged_stats(unsigned long long out[6]) {
  for (int i = 0; i < 6; i++) out[i] = g_attn_prefill_paged[i].load(std::memory_order_relaxed);
}

size_t ns_hip_attn_block_paged_workspace_size(int batch, int head_num, int heads_kv, int head_size, int max_q, int capacity) {
  return attn_block_paged_ws_bytes(attn_knobs(), batch, head_num, heads_kv, head_size, max_q, capacity);
}

void ns_hip_attn_block_paged_stats(unsigned long long out[4]) {
  for (int i = 0; i < 4; i++) out[i] = g_attn_block_paged[i].load(std::memory_order_relaxed);
}

void ns_hip_attn_paged_stats(unsigned long long out[4]) {
  for (int i = 0; i < 4; i++) out[i] = g_attn_paged[i].load(std::memory_order_relaxed);
}

void ns_hip_attn_rows_stats(unsigned long long out[4]) {
  for (int i = 0; i < 4; i++) out[i] = g_attn_rows[i].load(std::memory_order_relaxed);
}

}  // extern "C"
