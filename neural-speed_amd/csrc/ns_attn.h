// ns_attn.h — what the attention files share (internal).  Kernels: ns_attn_decode.hip (one query row per workgroup), ns_attn_prefill.hip (matrix
// cores), ns_attn_block.hip (matrix cores over context ranges: a short block of query rows over a long cache).  Host: ns_attn_plan.cpp decides which kernel serves a call (attn_plan: a pure function, checked on the CPU by tests/test_attn_plan.py),
// ns_attn.cpp reads the tunables, takes scratch and launches what the plan says.  ns_kvcache.hip is the library-managed kv-cache on top of them.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ns_bestla.h"
#include "ns_common.h"

namespace ns {

constexpr int kAttnThreads = 256;
constexpr int kAsSteps = 8;                                     // attn_stream_kernel: steps of a wave's ring
constexpr size_t kAsLdsBytes = size_t(4) * kAsSteps * 2048;    // ... and its LDS: [4 waves][kAsSteps][K image 1 KiB | V image 1 KiB]
constexpr int kA2KB = 64;                                       // attn_mfma2 / attn_mfma3_kernel: keys per tile
constexpr int kA2VSub = kA2KB * 32 + 128;                       // bytes per V subtile: [64 keys][16 dims] fp16 + the bank offset
template <int HS>
constexpr int a2_stage_bytes() { return kA2KB * HS * 2 + (HS / 16) * kA2VSub; }
constexpr size_t kAttnTicketCap = 65536;                        // merge tickets of a stream (SLOT_ATTN_TICKETS)

struct AttnParams {
  const float* q;
  const _Float16* k;
  const _Float16* v;
  float* dst;
  _Float16* dst16;  // optional fp16 shadow of dst (same element strides): the next GEMM's A operand
  float qk_scale;   // QK_scale * Q_sc * K_sc
  float out_scale;  // V_sc / dst_sc
  uint32_t flags;
  int head_num, heads_kv, head_size, sl_q, sl_kv;
  long long step_q_bs, step_q_head_num, step_q_sl;
  long long step_k_bs, step_k_head_num, step_k_sl, step_k_head_size;
  long long step_v_bs, step_v_head_num, step_v_sl, step_v_head_size;
  long long step_dst_bs, step_dst_head_num, step_dst_sl;
  int hs_pad;  // power of two >= head_size (<= 256)
  float alibi_m0, alibi_m1;
  int alibi_log2_floor;
  int alibi_head_off;  // tensor parallel: index of this rank's first head in the full model (0 otherwise)
};

struct AttnSplitParams {
  AttnParams a;
  float* ws;       // [batch][sl_q][head][nsplit][2 + head_size] partial (m, l, acc) when nsplit > 1
  int nsplit;
  int keys_per_split;
  uint32_t* tickets;  // one self-resetting counter per (batch, query row, kv head, chunk): the LAST split to finish merges inside the
                      // launch (nullptr: attn_merge_kernel does it in a second launch)
  int heads_first;     // 1: blockIdx.x walks the (kv head, row) pairs and blockIdx.y the context ranges — neighbouring workgroups then read
                       // neighbouring 256-byte pieces of a position-major cache ([position][head][dim]); 0: the ranges of one head first
  int g_full, chunks;  // query heads per kv head, and in how many workgroups of G heads each they are served (round 4: any head
                       // group — Falcon's 71 and StarCoder's 48 query heads on one kv head ran on the one-workgroup-per-head kernel)
  // replayed device route (round 6, ns_common.h Affine): the context length moves with the captured graph's token counter —
  // sl_kv = a.sl_kv + kdelta * *kmove.  Grid, keys_per_split and the partials' layout are those of the LONGEST context (nsplit ranges);
  // ranges past the live length leave at once, a single live range writes the output row itself, the merge reads the live ones only.
  const int* kmove;
  int kdelta;
  // ... and the ranges follow the LIVE length (round 6, second half): a plan laid out for n_ctx = 2048 (8 ranges of 256 keys) used to run 1530 cached positions
  // on 6 of its 8 workgroups per head, 600 positions on 3 — with n_ctx = 4096 half as many again.  Every workgroup applies the host's range rule
  // (attn_nsplit) to the live length itself: dyn_min_keys / dyn_batch_keys / dyn_single_below are that rule's constants for this launch, nsplit its
  // upper bound (grid and partials' layout stay those of the longest context).  dyn_min_keys == 0: ranges as laid out (keys_per_split).
  int dyn_min_keys, dyn_batch_keys, dyn_single_below;
  // A batch of independent requests (ns_hip_attn_decode_rows; AttnPlan::rows, the kernels' ROWS instantiations): the moving length is ONE VALUE PER
  // BATCH ENTRY — clamp(kmove[ibs] + kdelta, 0, a.sl_kv): kmove is an array, kdelta the bias added to its entries, a.sl_kv the capacity of a request's
  // slab.  Everything above holds per request (ranges, live ranges, the single live range that writes its row); a length of 0 is an idle slot, whose
  // output row the first range's workgroups write as zeros.  (No field of its own: the struct, and with it the code of every other instantiation,
  // is what it was.)
};
// live context length / live ranges of a launch (kmove == nullptr: what the host said).  Host and device: tests/test_attn_plan.py walks every live
// length of a plan through the two range functions.  ROWS: the per-request form, the live length of batch entry ibs (the clamp and the zero
// length belong to it alone) — a template argument, so the instantiations that serve every other call hold the code they held without it.
template <bool ROWS = false>
__host__ __device__ __forceinline__ int attn_live_kv(const AttnSplitParams& sp, int ibs = 0) {
  if constexpr (ROWS) {
    const long long len = (long long)sp.kmove[ibs] + sp.kdelta;
    return len < 0 ? 0 : (len > sp.a.sl_kv ? sp.a.sl_kv : int(len));
  }
  return sp.kmove ? sp.a.sl_kv + sp.kdelta * *sp.kmove : sp.a.sl_kv;
}
// keys per range at the live length (the host's rule: as many ranges as the launch has workgroups for, at least dyn_min_keys keys each, whole softmax batches)
__host__ __device__ __forceinline__ int attn_live_kps(const AttnSplitParams& sp, int sl_kv) {
  if (!sp.kmove || sp.dyn_min_keys <= 0) return sp.keys_per_split;
  if (sl_kv <= sp.dyn_single_below) return max(sl_kv, 1);
  const int want = max(1, min(sp.nsplit, (sl_kv + sp.dyn_min_keys - 1) / sp.dyn_min_keys));
  int kps = (sl_kv + want - 1) / want;
  if (sp.dyn_batch_keys > 1 && want > 1) kps = (kps + sp.dyn_batch_keys - 1) / sp.dyn_batch_keys * sp.dyn_batch_keys;
  return kps;
}
__host__ __device__ __forceinline__ int attn_live_splits(const AttnSplitParams& sp, int sl_kv) {
  if (!sp.kmove) return sp.nsplit;
  const int kps = attn_live_kps(sp, sl_kv);
  return max(1, (sl_kv + kps - 1) / kps);
}

// ---- a paged cache (ns_hip_attn_decode_paged, ns_hip_rope_qkv_append_paged, ns_hip_kv_paged_store) -------------------------------------------------
// K and V live in two pools of pool_blocks blocks of (1 << block_shift) keys; block b starts block_step elements behind block b - 1, inside a block a
// key's row is step_sl elements behind its predecessor's and a head's step_head_num behind the head before it (the caller's strides: position-major
// and head-major blocks are both expressible).  table[request][table_stride] (DEVICE memory) names the physical block of a request's logical block.
// The table is the caller's and read inside the launch, so nothing on the host can vouch for an entry: an id outside [0, pool_blocks) never becomes
// an address (attn_page_at answers -1).  Two requests may name the same block.
struct AttnPage {
  const int* table;
  int table_stride;  // entries per request: a request's capacity is table_stride << block_shift keys
  int block_shift;   // log2 of the keys per block (4 .. 8)
  int pool_blocks;
  long long block_step;
};
// block_keys -> block_shift; -1: not a power of two from 16 to 256 (which every entry refuses)
inline int attn_block_shift(int block_keys) {
  for (int s = 4; s <= 8; s++)
    if (block_keys == 1 << s) return s;
  return -1;
}
// Argument block of the PAGED instantiations: the fields are added AROUND AttnSplitParams, so every other instantiation's argument block is what it was.
struct AttnPagedParams {
  AttnSplitParams sp;
  AttnPage pg;
};
// Key n of a request -> its cell.  THE translation: the kernels, the append, the store and tests/tools/attn_paged_plan_main.cpp all go through these two.
// attn_page_at: the element offset, from the pool's base, of key n's row in physical block `blk` (head 0, dim 0; step_sl: K's or V's row stride), or
// -1 = no access: blk is not a block of the pool.
__host__ __device__ __forceinline__ long long attn_page_at(const AttnPage& pg, int blk, int n, long long step_sl) {
  if (unsigned(blk) >= unsigned(pg.pool_blocks)) return -1;
  return (long long)blk * pg.block_step + (long long)(n & ((1 << pg.block_shift) - 1)) * step_sl;
}
// attn_page_cell: the same for key n of request b through the table; -1 also for a key outside the request's capacity.
__host__ __device__ __forceinline__ long long attn_page_cell(const AttnPage& pg, int b, int n, long long step_sl) {
  const int j = n >> pg.block_shift;
  if (n < 0 || j >= pg.table_stride) return -1;
  return attn_page_at(pg, pg.table[(long long)b * pg.table_stride + j], n, step_sl);
}
// The ring kernel addresses a pool through ONE 32-bit buffer descriptor over the whole pool (offsets are never wrapped): a pool it cannot address is
// served by the register kernel, whose pointers are 64-bit.  256 elements of slack as in the slab rule (ns_attn_plan.cpp, attn_in32).
__host__ __device__ __forceinline__ bool attn_page_in32(const AttnPage& pg) {
  return ((unsigned long long)pg.pool_blocks * (unsigned long long)pg.block_step + 256ull) * 2ull < (1ull << 32);
}

// ---- ragged query blocks over a paged cache (ns_hip_attn_block_paged; attn_block_split_kernel's PAGED instantiations, ns_attn_block.hip) ---------
// Argument block: sp as the block-split kernel reads it, with a.sl_q = max_q (the most query rows of one request), a.sl_kv = a request's capacity,
// kmove / kdelta = dKvLens / its bias (attn_live_kv<true>), nsplit / keys_per_split = the ranges laid out for the capacity, dyn_min_keys = the block
// rule's least keys per range for the workgroups to apply to the live length (0: ranges as laid out).  q_start[requests + 1]: request b's query rows
// are the packed rows q_start[b] .. q_start[b + 1] - 1 of Q / dst.  Partials: ws[request][row of the request < max_q][head][nsplit][2 + head_size].
struct AttnBlockPagedParams {
  AttnSplitParams sp;
  AttnPage pg;
  const int* q_start;
};
// Keys per range and live ranges of a request with kv_len live keys, under a layout of nsplit ranges of kps_laid keys (a multiple of 64).  THE live
// rule of that entry: the range workgroups and the merge both go through it, tests/test_attn_block_paged_plan.py walks every live length through it.
// The ranges [i * kps, min((i + 1) * kps, kv_len)), i < live, tile [0, kv_len); kps is a multiple of 64 and live <= nsplit.
struct AttnBlockLive {
  int kps, live;
};
__host__ __device__ __forceinline__ AttnBlockLive attn_block_live(int kv_len, int nsplit, int kps_laid, int min_keys) {
  if (kv_len <= 0) return {kps_laid, 0};
  if (min_keys <= 0) return {kps_laid, (kv_len + kps_laid - 1) / kps_laid};
  const int want = min(nsplit, max(1, (kv_len + min_keys - 1) / min_keys));
  const int kps = ((kv_len + want - 1) / want + 63) / 64 * 64;
  return {kps, (kv_len + kps - 1) / kps};
}
// query rows of request b in this call: clamp(q_start[b + 1] - q_start[b], 0, max_q)
__host__ __device__ __forceinline__ int attn_block_q_len(const int* q_start, int b, int max_q) {
  const long long n = (long long)q_start[b + 1] - q_start[b];
  return n < 0 ? 0 : (n > max_q ? max_q : int(n));
}

// ---- prompt-sized query blocks over a paged cache (ns_hip_attn_prefill_paged; attn_mfma2_body's PAGED instantiations, ns_attn_prefill.hip) --------
// Argument block: a as the 128-row kernel reads it, with a.sl_q = max_q, a.sl_kv = a request's capacity, a.k / a.v the pool bases and no batch step
// (Q, dst and dst16 are packed through q_start, as above); kv_lens[b] + kdelta, clamped to [0, capacity], are request b's live keys.
struct AttnPrefillPagedParams {
  AttnParams a;
  AttnPage pg;
  const int* q_start;
  const int* kv_lens;
  int kdelta;
};
// live keys of request b: attn_live_kv<true>'s clamp
__host__ __device__ __forceinline__ int attn_prefill_kv_len(const int* kv_lens, int b, int kdelta, int cap) {
  const long long len = (long long)kv_lens[b] + kdelta;
  return len < 0 ? 0 : (len > cap ? cap : int(len));
}
// Row r of a 64-key tile that starts at pos0 -> the key whose cell a PAGED workgroup stages there: the row clamped to the request's last live key
// (kv_len >= 1), so no cell behind kv_len is read and the table entry is that key's, (key >> block_shift) < ceil(kv_len / block_keys).  THE row
// rule of that kernel: its fetch and tests/tools/attn_prefill_paged_plan_main.cpp both go through it, then through attn_page_at.
__host__ __device__ __forceinline__ int attn_prefill_tile_key(int pos0, int r, int kv_len) { return min(pos0 + r, kv_len - 1); }

// ---- the launch decision as a value (ns_attn_plan.cpp) -------------------------------------------------------------------------------------
// Every tunable the decision reads.  attn_knobs() (ns_attn.cpp) fills it from ns_hip_set_tuning's atomics and the environment.
struct AttnKnobs {
  int attn_stream = 1;         // "attn_stream" / NS_ATTN_STREAM: 1 = head sizes 40 .. 128 stream K / V through LDS rings, 0 = through registers
  int attn_mfma2_rows = 128;   // "attn_mfma2_rows" / NS_ATTN_MFMA2_ROWS: query rows from which the 128-row kernels serve a prefill
  int attn_inlaunch = 0;       // "attn_inlaunch" / NS_ATTN_INLAUNCH: 1 = the last context range to finish merges inside the launch
  int attn_heads_first = -1;   // "attn_heads_first" / NS_ATTN_HEADS_FIRST: dispatch order of a split launch, -1 = by the cache's layout
  int wg_target = 1024, min_keys = 128;     // "attn_wg_target" / "attn_min_keys": range rule of the register kernel
  int wg_target_s = 256, min_keys_s = 32;   // "attn_stream_wg_target" / "attn_stream_min_keys": ... of the ring kernel
  bool no_mfma = false;        // NS_ATTN_NO_MFMA set: no matrix-core kernel (diagnostics)
  int pipe = 1;                // NS_ATTN_PIPE: 0 = attn_mfma2_kernel where attn_mfma3_kernel would serve
  int pvar = -1;               // NS_ATTN_PVAR: schedule variant of attn_mfma3_kernel, -1 = by length
  bool no_xcd_map = false;     // NS_ATTN_NO_XCD_MAP set: plain workgroup order of the 128-row kernels (A/B)
  bool v1 = false;             // NS_ATTN_V1 set: attn_kernel where a split kernel would serve (diagnostics)
  bool dyn_ranges = true;      // NS_ATTN_DYN_RANGES=0: a moving context length keeps the ranges as laid out (A/B)
  int alibi_heads = 0, alibi_off = 0;  // ns_hip_attn_set_head_partition
  bool no_partials = false;    // not a tunable: launch_attn's second plan when the partials' scratch cannot be had — one range, still correct
  int block_split = 0;         // "attn_block_split" / NS_ATTN_BLOCK_SPLIT: > 0 = 2 .. 127 query rows over max(value, 256) or more keys take the
                               // context-split 64-slot kernel (attn_block_split_kernel); 0 (default) = every plan as without it
  int block_target = 512, block_min_keys = 128;  // "attn_block_wg_target" / "attn_block_min_keys": its range rule (scripts/attn_block_split_bench.py)
};
enum AttnPath { AP_REFUSED = 0, AP_GENERIC, AP_SPLIT_REGS, AP_RING, AP_ROWS64, AP_ROWS128, AP_PIPELINED, AP_BLOCK_SPLIT };
constexpr int kAttnPaths = 8;  // ns_hip_attn_stats: one counter per AttnPath value
// What a launch needs; nothing is decided after it.  sp.ws and sp.tickets are null: the launcher's scratch.
struct AttnPlan {
  AttnPath path = AP_REFUSED;
  int G = 0, lpk = 0, dpl = 0;       // one-row paths: attn_split_kernel<G, dpl> / attn_stream_kernel<G, lpk>
  int hs_pad = 0, sb = 0, pad = 0;   // matrix-core paths: attn_mfma_kernel<hs_pad> / attn_mfma2(_hs256)_kernel<hs_pad, sb, pad> / attn_mfma3_kernel<hs_pad> /
                                     // attn_block_split_kernel<hs_pad> (which reads sp.nsplit, sp.keys_per_split and sp.g_full as well)
  AttnSplitParams sp;                // sp.a: the kernels' AttnParams; the rest (ranges, order, head groups, moving length): one-row paths
  dim3 grid, block;
  size_t lds = 0;                    // dynamic LDS bytes
  bool rows = false;                 // one-row paths: one live length per batch entry (the ROWS instantiations; sp.kmove an array, sp.kdelta its bias)
  bool paged = false;                // ... over a paged cache (the PAGED instantiations; page: their AttnPage, sp.a.k / sp.a.v the pool bases)
  AttnPage page = {};
  bool want_tickets = false;         // ranges merge inside the launch if the stream's ticket buffer can be had
  bool merge = false;                // attn_merge_kernel follows (also when tickets are wanted and cannot be had)
  size_t partial_bytes = 0;          // of sp.ws
  int nqb = 0, aligned = 0, xcd_map = 0;  // 128-row paths: query blocks per head, 16-byte stores of the output, XCD remap | variant << 8
};
bool attn_shape_ok(int head_num, int heads_kv, int head_size, int sl_q, int sl_kv, bool causal, std::string* why);
// dst16: the optional fp16 shadow of dst (its alignment is part of the decision).  AP_REFUSED: *why says what is wrong with the call.
// page != nullptr (with aff.rows): K / V are the pools of a paged cache — the plan of the per-request form of the same shape and capacity, plus the paging's
// own refusals and the 32-bit rule of the pool (attn_page_in32) in place of the slab's.
AttnPlan attn_plan(const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, const void* dst16, const AttnKnobs& knobs, const Affine& aff, std::string* why,
                   const AttnPage* page = nullptr);
// what bestla_fusion_attn_workspace_size answers: it knows neither strides nor alignment, so the most any plan of the shape can need
size_t attn_ws_bytes(const AttnKnobs& knobs, int batch, int head_num, int heads_kv, int head_size, int sl_q, int sl_kv);

// The plan of ns_hip_attn_block_paged: a pure function like attn_plan (tests/test_attn_block_paged_plan.py).  a.sl_q is max_q, a.sl_kv the capacity.
// Ranges: the block rule of AP_BLOCK_SPLIT (kn.block_target / kn.block_min_keys) for the capacity and max_q rows of every request; kn.dyn_ranges:
// the workgroups apply it to their request's live length.  !ok: *why says what is wrong with the call.  pp.sp.ws is null: the launcher's scratch.
struct AttnBlockPagedPlan {
  bool ok = false;
  int hs_pad = 0;
  AttnBlockPagedParams pp;
  dim3 grid, block, merge_grid;  // (slot blocks of max_q rows * kv heads, nsplit, requests) x 256; (heads, max_q, requests) x 128
  size_t partial_bytes = 0;
};
AttnBlockPagedPlan attn_block_paged_plan(const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, const void* dst16, const AttnKnobs& knobs, const AttnPage& page,
                                         const int* q_start, const int* kv_lens, int kv_len_bias, std::string* why);
// what ns_hip_attn_block_paged_workspace_size answers: the plan's partial_bytes, from the shape alone (0: no plan of that shape)
size_t attn_block_paged_ws_bytes(const AttnKnobs& knobs, int batch, int head_num, int heads_kv, int head_size, int max_q, int capacity);

// The plan of ns_hip_attn_prefill_paged: a pure function like attn_block_paged_plan (tests/test_attn_prefill_paged_plan.py).  a.sl_q is max_q, a.sl_kv
// the capacity.  One launch of attn_mfma2_body<hs_pad, sb, pad, 1, PAGED>: ceil(max_q / 128) query blocks x heads x requests workgroups; the query
// blocks a request does not have leave at once.  No partials, no scratch.  !ok: *why says what is wrong with the call.
struct AttnPrefillPagedPlan {
  bool ok = false;
  int hs_pad = 0, sb = 0, pad = 0;  // the template arguments
  AttnPrefillPagedParams pp;
  dim3 grid, block;
  size_t lds = 0;
  int nqb = 0, aligned = 0, xcd_map = 0;  // query blocks per (head, request), 16-byte stores of the output, XCD remap
};
AttnPrefillPagedPlan attn_prefill_paged_plan(const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, const void* dst16, const AttnKnobs& knobs, const AttnPage& page,
                                             const int* q_start, const int* kv_lens, int kv_len_bias, std::string* why);

// ---- launches of a plan ----------------------------------------------------------------------------------------------------------------------
hipError_t launch_attn_onerow(const AttnPlan& pl, float* ws, uint32_t* tickets, hipStream_t st);  // ns_attn_decode.hip: AP_GENERIC, AP_SPLIT_REGS, AP_RING (+ merge)
hipError_t launch_attn_rows(const AttnPlan& pl, hipStream_t st);                                  // ns_attn_prefill.hip: AP_ROWS64, AP_ROWS128, AP_PIPELINED
hipError_t launch_attn_block_split(const AttnPlan& pl, float* ws, hipStream_t st);                // ns_attn_block.hip: AP_BLOCK_SPLIT (+ merge)
hipError_t launch_attn_block_paged(const AttnBlockPagedPlan& pl, float* ws, hipStream_t st);     // ns_attn_block.hip: the PAGED instantiation + its merge
hipError_t launch_attn_prefill_paged(const AttnPrefillPagedPlan& pl, hipStream_t st);             // ns_attn_prefill.hip: the PAGED instantiations of the 128-row kernel
hipError_t launch_attn_merge(const AttnSplitParams& sp, unsigned batch, hipStream_t st, bool rows = false);  // ns_attn_decode.hip: attn_merge_kernel over sp.ws
// touch_attn_module (ns_common.h) makes the runtime load all four code objects
inline void touch_kernel(const void* kernel) {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, kernel);
  (void)hipGetLastError();
}
void touch_attn_rows_module();  // ns_attn_prefill.hip
void touch_attn_block_module(); // ns_attn_block.hip
void touch_kvcache_module();    // ns_kvcache.hip
// Is a HIP device visible?  who != nullptr: if not, the error is set and "Err: invalid parameters (<who>: no HIP device visible ...)" goes to stderr.
bool attn_device_visible(const char* who);

}  // namespace ns
