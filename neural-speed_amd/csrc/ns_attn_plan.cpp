// ns_attn_plan.cpp — which kernel serves an attention call, as a value.  attn_plan is a pure function of the call, the tunables and the moving
// context length of a replayed route: no HIP call, no environment, no global, no scratch — tests/test_attn_plan.py runs it on the CPU over a grid
// of cases against the table of docs/kernels/attention.md ("What tests which launch path").  Each rule is stated once, here.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ns_attn.h"

namespace ns {

bool attn_shape_ok(int head_num, int heads_kv, int head_size, int sl_q, int sl_kv, bool causal, std::string* why) {
  if (head_size < 1 || head_size > 256) {
    *why = "attention: head_size must be 1..256";
    return false;
  }
  if (heads_kv < 1 || head_num % heads_kv != 0) {
    *why = "attention: head_num must be a multiple of heads_kv";
    return false;
  }
  if (causal && sl_q > sl_kv) {
    *why = "attention: causal needs sl_q <= sl_kv";
    return false;
  }
  if (sl_q < 1 || sl_kv < 1) {
    *why = "attention: empty sequence";
    return false;
  }
  return true;
}

// query heads per workgroup of the split kernels (their template argument) and workgroups per kv head for a head group of g_full
static void attn_groups(int g_full, int* G, int* chunks) {
  *G = g_full <= 1 ? 1 : (g_full == 2 ? 2 : (g_full <= 4 ? 4 : 8));
  *chunks = (g_full + *G - 1) / *G;
}

// ---- context ranges of a one-row launch ------------------------------------------------------------------------------------------------------
// The register kernel aims at ~4 workgroups per CU with at least 128 keys per range.  The LDS-ring kernel has its own rule
// (profiles/r05p_attn_stream.txt): a workgroup keeps 64 KiB in flight whatever its range, so ONE workgroup per CU streams best — 32 kv heads at
// 2048 positions: 8 ranges of 256 keys 12.9 us (split + merge) against 13.7 with 16 x 128 and 15.2 with 32 x 64; 8 kv heads: 32 ranges of 64 keys
// 13.5 us against 16.6 with 16 x 128 (128 workgroups: half the chip idle).
// batch_keys (ring kernel): keys one softmax update of a workgroup covers (U steps); a range that is not a multiple of it computes masked key slots,
// which costs where the update is VALU-heavy (8 query heads per workgroup: Falcon-7B's 71 heads on one kv head at 2048 keys, 29 ranges of 71 keys
// 32.5 us against 16 x 128 keys 28.5) — ranges are rounded up to it while that leaves at least 128 workgroups.
// heavy (workgroups that serve 4 or 8 query heads per key: twice the arithmetic per byte): two workgroups per CU overlap better than one once a batch
// brings 64+ workgroups per range — batch 8 x 32 / 8 heads at 2048 keys 36.7 -> 32.0 us, batch 16 64.0 -> 50.5 (scripts/r05/attn_batch_rule.py).
// single_below: a range's worth of keys on 32+ workgroups stays one range (the merge launch costs more than it saves, 7.0 vs 7.8 us).
// min_keys, batch_keys and single_below are also what the workgroups of a moving-length launch apply to the live length (attn_live_kps).
struct RangeRule {
  int target, min_keys, batch_keys, single_below;
};
static RangeRule range_rule(const AttnKnobs& kn, size_t base_blocks, bool ring, int batch_keys, bool heavy) {  // base_blocks: workgroups per range
  RangeRule r;
  r.target = ring ? kn.wg_target_s : kn.wg_target;
  if (ring && heavy && base_blocks >= 64) r.target *= 2;
  r.min_keys = ring ? kn.min_keys_s : kn.min_keys;
  r.batch_keys = ring ? batch_keys : 0;
  r.single_below = ring && base_blocks >= 32 ? 128 : 0;
  return r;
}
static int attn_nsplit(const RangeRule& r, size_t base_blocks, int sl_kv) {
  if (sl_kv <= r.single_below) return 1;
  int nsplit = int((r.target + base_blocks - 1) / base_blocks);
  nsplit = std::min(nsplit, std::max(1, (sl_kv + r.min_keys - 1) / r.min_keys));
  nsplit = std::min(nsplit, 64);
  if (r.batch_keys > 0 && nsplit > 1) {
    const int kps = ((sl_kv + nsplit - 1) / nsplit + r.batch_keys - 1) / r.batch_keys * r.batch_keys;
    const int rounded = (sl_kv + kps - 1) / kps;
    if (size_t(rounded) * base_blocks >= 128) nsplit = rounded;
  }
  return nsplit;
}
// partials of nsplit ranges: [batch][sl_q][head][nsplit][2 + head_size] floats
static size_t attn_partial_bytes(int batch, int sl_q, int head_num, int head_size, int nsplit) {
  return nsplit > 1 ? size_t(batch) * sl_q * head_num * nsplit * (2 + head_size) * 4 : 0;
}
size_t attn_ws_bytes(const AttnKnobs& kn, int batch, int head_num, int heads_kv, int head_size, int sl_q, int sl_kv) {
  int G, chunks;
  attn_groups(head_num / std::max(1, heads_kv), &G, &chunks);
  const size_t bb = size_t(heads_kv) * chunks * sl_q * batch;
  int ns = 1;  // any rule a plan of this shape can take
  for (int rule = 0; rule < 3; rule++) ns = std::max(ns, attn_nsplit(range_rule(kn, bb, rule > 0, 0, rule == 2), bb, sl_kv));
  return attn_partial_bytes(batch, sl_q, head_num, head_size, ns);
}

// K / V rows of a head lie inside a 32-bit buffer descriptor (the DMA kernels: attn_stream_kernel, attn_mfma3_kernel)
static bool attn_in32(int sl_kv, long long step_k_sl, long long step_v_sl) {
  return (size_t(sl_kv) * size_t(step_k_sl) + 256) * 2 < (size_t(1) << 32) && (size_t(sl_kv) * size_t(step_v_sl) + 256) * 2 < (size_t(1) << 32);
}

// What a paged call must satisfy beyond the per-request form (ns_hip_attn_decode_paged); nullptr: nothing to say against it.
// The last rule is what makes every cell of a valid block id an address inside the pool: a block holds its keys' rows of every kv head.
static const char* attn_page_refusal(const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, const AttnPage& pg) {
  if (!pg.table) return "attention, paged cache: the block table is null";
  if (pg.block_shift < 4 || pg.block_shift > 8) return "attention, paged cache: block_keys must be a power of two from 16 to 256";  // (attn_block_shift)
  const int block_keys = 1 << pg.block_shift;
  if (pg.pool_blocks < 1) return "attention, paged cache: pool_blocks must be at least 1";
  if (pg.table_stride < 1 || (long long)pg.table_stride * block_keys != a.sl_kv)
    return "attention, paged cache: sl_kv is the capacity of a request and must equal table_stride * block_keys";
  if (pg.block_step < 1 || pg.block_step % 8 != 0) return "attention, paged cache: block_step must be a positive multiple of 8 elements (16-byte aligned blocks)";
  const long long last = (long long)(block_keys - 1);
  if (a.step_k_sl < 0 || a.step_v_sl < 0 || a.step_k_head_num < 0 || a.step_v_head_num < 0 ||
      last * a.step_k_sl + (long long)(a.heads_kv - 1) * a.step_k_head_num + a.head_size > pg.block_step ||
      last * a.step_v_sl + (long long)(a.heads_kv - 1) * a.step_v_head_num + a.head_size > pg.block_step)
    return "attention, paged cache: a block's keys and kv heads (step_k / step_v strides) do not fit inside block_step";
  return nullptr;
}

AttnPlan attn_plan(const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, const void* dst16, const AttnKnobs& kn, const Affine& aff, std::string* why,
                   const AttnPage* page) {
  AttnPlan pl;
  memset(&pl.sp, 0, sizeof(pl.sp));
  auto refuse = [&](const char* text) {
    *why = text;
    return pl;
  };
  if (a.Q_layout != ATTN_FWD_LAYOUT_PLAIN || a.K_layout != ATTN_FWD_LAYOUT_PLAIN || a.V_layout != ATTN_FWD_LAYOUT_PLAIN ||
      a.dst_layout != ATTN_FWD_LAYOUT_PLAIN)
    return refuse("attention: only ATTN_FWD_LAYOUT_PLAIN tensors are supported");
  if (!attn_shape_ok(a.head_num, a.heads_kv, a.head_size, a.sl_q, a.sl_kv, (a.attn_flags & NS_ATTN_FLAG_IS_CAUSAL) != 0, why)) return pl;
  AttnParams& p = pl.sp.a;
  p.q = a.Q;
  p.k = reinterpret_cast<const _Float16*>(a.K);
  p.v = reinterpret_cast<const _Float16*>(a.V);
  p.dst = a.dst;
  p.dst16 = static_cast<_Float16*>(const_cast<void*>(dst16));
  p.qk_scale = a.QK_scale * a.Q_sc * a.K_sc;
  p.out_scale = a.V_sc / a.dst_sc;
  p.flags = a.attn_flags;
  p.head_num = a.head_num, p.heads_kv = a.heads_kv, p.head_size = a.head_size, p.sl_q = a.sl_q, p.sl_kv = a.sl_kv;
  p.step_q_bs = a.step_q_bs, p.step_q_head_num = a.step_q_head_num, p.step_q_sl = a.step_q_sl;
  p.step_k_bs = a.step_k_bs, p.step_k_head_num = a.step_k_head_num, p.step_k_sl = a.step_k_sl;
  p.step_k_head_size = a.step_k_head_size;
  p.step_v_bs = a.step_v_bs, p.step_v_head_num = a.step_v_head_num, p.step_v_sl = a.step_v_sl;
  p.step_v_head_size = a.step_v_head_size;
  p.step_dst_bs = a.step_dst_bs, p.step_dst_head_num = a.step_dst_head_num, p.step_dst_sl = a.step_dst_sl;
  p.hs_pad = a.head_size <= 64 ? 64 : (a.head_size <= 128 ? 128 : 256);
  // mha_dense_wrapper.h:1418-1447: under tensor parallelism the slopes follow the FULL model's head count and this
  // rank's first head (the reference takes world/rank from parallel_context; here ns_hip_attn_set_head_partition)
  const int all_heads = kn.alibi_heads > 0 ? kn.alibi_heads : a.head_num;
  p.alibi_head_off = kn.alibi_heads > 0 ? kn.alibi_off : 0;
  if (p.alibi_head_off < 0 || p.alibi_head_off + a.head_num > all_heads)
    return refuse("attention: head partition (ns_hip_attn_set_head_partition) does not contain this call's heads");
  const int lf = 1 << int(floor(log2(double(all_heads))));
  p.alibi_log2_floor = lf;
  p.alibi_m0 = powf(2.0f, -8.f / float(lf));
  p.alibi_m1 = powf(2.0f, -4.f / float(lf));
  if (a.head_num > 65535 || a.batch_size > 65535) return refuse("attention: head_num / batch_size above the grid limit");
  // replayed device route (ns_route.cpp): the context length of a captured decode step moves with the graph's token counter
  if (aff.k && (a.sl_q != 1 || aff.cap < a.sl_kv))
    return refuse("attention: a moving context length is served for decode steps (one query row) within the cache's capacity");
  if (aff.k && aff.rows && aff.cap != a.sl_kv) return refuse("attention: per-request context lengths take sl_kv as the capacity of a request's slab");
  // a paged cache (ns_hip_attn_decode_paged): the per-request form with K / V as pools; the batch strides of K / V are not used
  if (page) {
    if (!aff.k || !aff.rows) return refuse("attention, paged cache: served for per-request context lengths only");
    if (const char* text = attn_page_refusal(a, *page)) return refuse(text);
    pl.paged = true, pl.page = *page;
    p.step_k_bs = p.step_v_bs = 0;  // (the kernels add ibs * step_bs to the pools' bases)
  }
  // what every kernel but attn_kernel asks of K and V: a contiguous head dimension and 16-byte aligned rows
  const bool rows_ok = a.step_k_head_size == 1 && a.step_v_head_size == 1 && a.step_k_sl % 8 == 0 && a.step_v_sl % 8 == 0 &&
                       a.step_k_head_num % 8 == 0 && a.step_v_head_num % 8 == 0 && (page || (a.step_k_bs % 8 == 0 && a.step_v_bs % 8 == 0)) && (reinterpret_cast<uintptr_t>(a.K) & 15) == 0 &&
                       (reinterpret_cast<uintptr_t>(a.V) & 15) == 0;

  const bool biased = (a.attn_flags & (NS_ATTN_FLAG_IS_ALIBI8 | NS_ATTN_FLAG_IS_TANH30)) != 0;
  // ---- a short block of query rows over a long cache: matrix cores over context ranges (opt-in, kn.block_split) ----
  // A workgroup serves 64 SLOTS of one kv head — slot = row * g_full + j is query row `row` of the head group's j-th query head — over one range of
  // keys, so K / V of a kv head are read once per slot block and range, whatever the head group; attn_merge_kernel combines the ranges.
  // Ranges: two workgroups per CU, two 64-key blocks or more per range, whole blocks (512 / 128: the best pair of {128, 256, 512} x {128, 256} over
  // 4 / 16 / 64 rows x 2048 / 8192 keys x 32 / 8 kv heads, profiles/attn_block_split.txt; 256 / 128, the ring kernel's pair, is 5 % behind).
  if (kn.block_split > 0 && a.sl_q >= 2 && a.sl_q <= 127 && (a.head_size == 64 || a.head_size == 128) && !biased && rows_ok && !aff.k && !kn.no_mfma &&
      !kn.v1 && !kn.no_partials && a.sl_kv >= std::max(kn.block_split, 256)) {
    const int g_full = a.head_num / a.heads_kv;
    const size_t slot_blocks = (size_t(a.sl_q) * g_full + 63) / 64;
    const size_t base = size_t(a.heads_kv) * slot_blocks * a.batch_size;
    int nsplit = int((size_t(std::max(1, kn.block_target)) + base - 1) / base);
    const int min_keys = std::max(1, kn.block_min_keys);
    nsplit = std::min(std::min(nsplit, std::max(1, (a.sl_kv + min_keys - 1) / min_keys)), 64);
    const int kps = ((a.sl_kv + nsplit - 1) / nsplit + 63) / 64 * 64;
    nsplit = (a.sl_kv + kps - 1) / kps;  // (no range starts at or past sl_kv)
    if (size_t(a.heads_kv) * slot_blocks <= 65535 && nsplit >= 2) {
      pl.path = AP_BLOCK_SPLIT;
      pl.hs_pad = p.hs_pad;
      pl.grid = dim3(unsigned(slot_blocks * a.heads_kv), unsigned(nsplit), unsigned(a.batch_size));
      pl.block = dim3(256);
      pl.sp.nsplit = nsplit, pl.sp.keys_per_split = kps, pl.sp.g_full = g_full;
      pl.partial_bytes = attn_partial_bytes(a.batch_size, a.sl_q, a.head_num, a.head_size, nsplit);
      pl.merge = true;
      return pl;
    }
  }

  // ---- several query rows: matrix cores ----
  const size_t nqb = (size_t(a.sl_q) + 127) / 128, wgs2 = nqb * a.head_num * a.batch_size;
  // the 128-row kernels pad any head size that is a multiple of 8 to 64 / 128 / 256; the 64-row kernel takes 64 and 128 as they are and has no biased
  // form.  Shapes it cannot take use the 128-row kernels from 16 rows on: a workgroup with idle waves is still far from the one-row-per-workgroup
  // kernel they would fall to.  The 128-row kernels take the maximum of RAW scores: other score scales than positive ones go to the 64-row kernel.
  const bool exact = a.head_size == 64 || a.head_size == 128;
  const bool only128 = biased || !exact;
  const bool rows128 = a.sl_q >= (only128 ? 16 : kn.attn_mfma2_rows) && wgs2 < (size_t(1) << 31) && (biased || p.qk_scale > 0.f);
  if (!kn.no_mfma && a.sl_q >= 16 && a.head_size % 8 == 0 && a.head_size <= 256 && rows_ok && (!only128 || rows128)) {
    pl.block = dim3(256);
    pl.hs_pad = p.hs_pad;
    if (!rows128) {  // 64-row workgroups, 16x16x32 MFMA (attn_mfma_kernel)
      pl.path = AP_ROWS64;
      pl.grid = dim3(unsigned((a.sl_q + 63) / 64), unsigned(a.head_num), unsigned(a.batch_size));
      return pl;
    }
    // 128-row workgroups, 32x32x16 MFMA, K / V tiles shared through LDS
    pl.nqb = int(nqb);
    pl.grid = dim3(unsigned(wgs2));
    pl.aligned = (reinterpret_cast<uintptr_t>(a.dst) & 15) == 0 && a.step_dst_sl % 4 == 0 && a.step_dst_head_num % 4 == 0 &&
                 a.step_dst_bs % 4 == 0 && (!dst16 || (reinterpret_cast<uintptr_t>(dst16) & 7) == 0);
    pl.sb = biased;
    pl.pad = !exact && a.head_size != 256;
    pl.lds = size_t(2) * (pl.hs_pad == 64 ? a2_stage_bytes<64>() : pl.hs_pad == 128 ? a2_stage_bytes<128>() : a2_stage_bytes<256>());
    pl.xcd_map = !kn.no_xcd_map && (size_t(a.heads_kv) * a.batch_size) % 8 == 0;
    // round 6: K / V tiles by DMA (attn_mfma3_kernel) for the exact head sizes without score bias, rows inside a 32-bit buffer descriptor; NS_ATTN_PIPE=0:
    // attn_mfma2_kernel.  Variant (NS_ATTN_PVAR): bit 0 = the next tile is requested behind K.Q^T instead of in front of it, bit 1 = raised priority while
    // K.Q^T issues — both gain from 4096 keys on (601-611 vs 558-585 TFLOPS causal, 742-751 vs 722 at 8192) and lose below (519-525 vs 529-530 at 2048)
    // (the rule over WHOLE tiles: attn_mfma3_kernel requests every row of its last 64-key tile, and the rows past the last key read as zeros only
    // while their 32-bit offsets do not wrap back into the descriptor — their weights are 0, but 0 x whatever lies there is not)
    if (kn.pipe && !biased && exact && attn_in32((a.sl_kv + kA2KB - 1) / kA2KB * kA2KB, a.step_k_sl, a.step_v_sl)) {
      pl.path = AP_PIPELINED;
      pl.xcd_map |= (kn.pvar >= 0 ? kn.pvar : (a.sl_kv >= 3072 ? 3 : 0)) << 8;
    } else {
      pl.path = AP_ROWS128;
    }
    return pl;
  }

  // ---- one query row per workgroup ----
  pl.block = dim3(kAttnThreads);
  int G, chunks;
  attn_groups(a.head_num / a.heads_kv, &G, &chunks);
  const int dpl = a.head_size <= 128 ? 8 : 16;  // head dims per lane of the register kernel
  const size_t base_blocks = size_t(a.heads_kv) * a.sl_q * chunks;  // workgroups per range and batch entry
  if (kn.v1 || !rows_ok || a.head_size % dpl != 0 || base_blocks > 65535) {
    // per-request context lengths (ns_hip_attn_decode_rows): attn_kernel knows one length per launch
    if (aff.rows && !rows_ok) return refuse("attention: per-request context lengths need K / V rows contiguous in the head dimension and 16-byte aligned");
    if (aff.rows) return refuse("attention: per-request context lengths need a head size that is a multiple of 8 and at most 65535 kv heads (and no NS_ATTN_V1)");
    pl.path = AP_GENERIC;
    pl.grid = dim3(unsigned(a.sl_q), unsigned(a.head_num), unsigned(a.batch_size));
    return pl;
  }
  AttnSplitParams& sp = pl.sp;
  sp.g_full = a.head_num / a.heads_kv, sp.chunks = chunks;
  const int rule_kv = aff.k ? int(aff.cap) : a.sl_kv;  // (moving length: ranges, partials and descriptors laid out for the longest context)
  // the LDS rings: head sizes 40 .. 128 (72 .. 128: sixteen lanes per key; 40 .. 64: eight — with sixteen, half of a request's lanes would carry
  // nothing: measured slower from 4096 positions on), row offsets inside a 32-bit buffer descriptor, 16-byte query loads
  const bool q16 = (reinterpret_cast<uintptr_t>(a.Q) & 15) == 0 && a.step_q_bs % 4 == 0 && a.step_q_head_num % 4 == 0 && a.step_q_sl % 4 == 0;
  // (a paged cache: the ring kernel's descriptor spans the pool — attn_page_in32 in place of the slab's rule; a larger pool takes the register kernel)
  const bool in32 = page ? attn_page_in32(*page) : attn_in32(rule_kv, a.step_k_sl, a.step_v_sl);
  const bool stream = a.head_size > 32 && a.head_size <= 128 && in32 && q16 && kn.attn_stream != 0;
  const int lpk = a.head_size > 64 ? 16 : 8;
  const int batch_keys = (G * 8 <= 16 ? 4 : 2) * 4 * (64 / lpk);  // attn_stream_kernel's U x keys per workgroup step
  // head sizes above 128 (register kernel, 16 dims per lane) take the ring kernel's range rule too: 16 x 256 heads 14.6 -> 10.4 us at 512 keys,
  // 51.8 -> 36.5 at 8192; 8 heads on one kv head 51 -> 40 at 2048 (scripts/r05/attn_regs_rule.py; head sizes <= 32 lose with it at 2048+ keys)
  const RangeRule rule = range_rule(kn, base_blocks * a.batch_size, stream || a.head_size > 128, stream ? batch_keys : 0, stream && G >= 4);
  const int nsplit = kn.no_partials ? 1 : attn_nsplit(rule, base_blocks * a.batch_size, rule_kv);
  sp.nsplit = nsplit;
  sp.keys_per_split = (rule_kv + nsplit - 1) / nsplit;
  pl.rows = aff.k && aff.rows;  // (one live length per batch entry: kdelta is the bias of the entries, a.sl_kv the capacity)
  sp.kmove = aff.k, sp.kdelta = pl.rows ? aff.bias : int(aff.delta);
  if (aff.k && nsplit > 1 && kn.dyn_ranges && a.sl_q == 1)  // the rule's constants, for the workgroups to apply to the live length
    sp.dyn_min_keys = rule.min_keys, sp.dyn_batch_keys = rule.batch_keys, sp.dyn_single_below = rule.single_below;
  // partials go to the caller's workspace (`tmp`, sized by bestla_fusion_attn_workspace_size) or the stream's scratch
  pl.partial_bytes = attn_partial_bytes(a.batch_size, a.sl_q, a.head_num, a.head_size, nsplit);
  // (the replayed route merges inside the launch: one launch less per layer of a token that is all launches — profiles/r05r_*)
  pl.want_tickets = nsplit > 1 && (kn.attn_inlaunch != 0 || (aff.k && aff.inlaunch)) && base_blocks * a.batch_size <= kAttnTicketCap;
  pl.merge = nsplit > 1 && !pl.want_tickets;
  // dispatch order (round 5, profiles/r05m_attn_layout_order_ab.txt): on a position-major cache ([position][head][dim]: a head's rows are
  // pieces one position stride apart) neighbouring workgroups should be neighbouring HEADS of one context range — split + merge 14.3 -> 13.7 us
  // at 2048 positions, 22.0 -> 19.9 at 4096 (Llama-2-7B shape); on a head-major cache (one slab per head) the ranges of one head first
  // (20.7 vs 23.4 us at 4096).  ns_hip_set_tuning("attn_heads_first", 0 / 1) forces one, -1 = by layout.
  sp.heads_first = kn.attn_heads_first < 0 ? a.step_k_head_num < a.step_k_sl : kn.attn_heads_first != 0;
  pl.grid = sp.heads_first ? dim3(unsigned(base_blocks), unsigned(nsplit), unsigned(a.batch_size))
                           : dim3(unsigned(nsplit), unsigned(base_blocks), unsigned(a.batch_size));
  pl.path = stream ? AP_RING : AP_SPLIT_REGS;
  pl.G = G, pl.lpk = stream ? lpk : 16, pl.dpl = stream ? 8 : dpl;
  pl.lds = stream ? kAsLdsBytes : size_t(4) * G * 16 * dpl * 4;  // the ring / attn_split_finish's acc_s: [4 waves][G][16 * dpl] floats
  return pl;
}

// ---- ragged query blocks over a paged cache (ns_hip_attn_block_paged) ------------------------------------------------------------------------------
// The ranges of the 64-slot kernel for `requests` requests of up to max_q rows over `cap` keys: AP_BLOCK_SPLIT's rule above (two workgroups per CU,
// kn.block_min_keys keys or more per range, whole 64-key blocks, no range that starts at or past cap), without its "two ranges or more" condition —
// this entry has no other kernel to give a call to, one range is a plan like any other.
static void block_paged_ranges(const AttnKnobs& kn, int requests, int heads_kv, int g_full, int max_q, int cap, size_t* slot_blocks, int* nsplit, int* kps) {
  *slot_blocks = (size_t(max_q) * g_full + 63) / 64;
  const size_t base = size_t(heads_kv) * *slot_blocks * requests;
  int ns = int((size_t(std::max(1, kn.block_target)) + base - 1) / base);
  const int min_keys = std::max(1, kn.block_min_keys);
  ns = std::min(std::min(ns, std::max(1, (cap + min_keys - 1) / min_keys)), 64);
  *kps = ((cap + ns - 1) / ns + 63) / 64 * 64;
  *nsplit = (cap + *kps - 1) / *kps;
}
// what the shape alone can say against a call (the workspace size function knows nothing else)
static const char* block_paged_shape_refusal(int requests, int head_num, int heads_kv, int head_size, int max_q, int cap) {
  if (requests < 1 || requests > 65535) return "attention, query blocks over a paged cache: batch_size (the requests) must be 1 .. 65535";
  if (head_size != 64 && head_size != 128) return "attention, query blocks over a paged cache: head_size must be 64 or 128";
  if (heads_kv < 1 || head_num < 1 || head_num % heads_kv != 0 || head_num > 65535)
    return "attention, query blocks over a paged cache: head_num must be a multiple of heads_kv (at most 65535)";
  if (max_q < 1 || max_q > 65535) return "attention, query blocks over a paged cache: sl_q is max_q, the most query rows of one request (1 .. 65535)";
  if (cap < 1) return "attention, query blocks over a paged cache: sl_kv is the capacity of a request (at least 1 key)";
  if (size_t(heads_kv) * ((size_t(max_q) * (head_num / heads_kv) + 63) / 64) > 65535)
    return "attention, query blocks over a paged cache: heads_kv * ceil(max_q * (head_num / heads_kv) / 64) above the grid limit of 65535";
  return nullptr;
}
size_t attn_block_paged_ws_bytes(const AttnKnobs& kn, int batch, int head_num, int heads_kv, int head_size, int max_q, int capacity) {
  if (block_paged_shape_refusal(batch, head_num, heads_kv, head_size, max_q, capacity)) return 0;
  size_t slot_blocks;
  int nsplit, kps;
  block_paged_ranges(kn, batch, heads_kv, head_num / heads_kv, max_q, capacity, &slot_blocks, &nsplit, &kps);
  return size_t(batch) * max_q * head_num * nsplit * (2 + head_size) * 4;
}
AttnBlockPagedPlan attn_block_paged_plan(const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, const void* dst16, const AttnKnobs& kn, const AttnPage& page,
                                         const int* q_start, const int* kv_lens, int kv_len_bias, std::string* why) {
  AttnBlockPagedPlan pl;
  memset(&pl.pp, 0, sizeof(pl.pp));
  auto refuse = [&](const char* text) {
    *why = text;
    return pl;
  };
  if (a.Q_layout != ATTN_FWD_LAYOUT_PLAIN || a.K_layout != ATTN_FWD_LAYOUT_PLAIN || a.V_layout != ATTN_FWD_LAYOUT_PLAIN ||
      a.dst_layout != ATTN_FWD_LAYOUT_PLAIN)
    return refuse("attention: only ATTN_FWD_LAYOUT_PLAIN tensors are supported");
  if (!q_start) return refuse("attention, query blocks over a paged cache: dQStart is null");
  if (!kv_lens) return refuse("attention, query blocks over a paged cache: dKvLens is null");
  if (const char* text = block_paged_shape_refusal(a.batch_size, a.head_num, a.heads_kv, a.head_size, a.sl_q, a.sl_kv)) return refuse(text);
  if (a.attn_flags & (NS_ATTN_FLAG_IS_ALIBI8 | NS_ATTN_FLAG_IS_TANH30))
    return refuse("attention, query blocks over a paged cache: ALiBi and the tanh cap are not served");
  if (const char* text = attn_page_refusal(a, page)) return refuse(text);
  // what the kernel asks of K and V, as every split kernel does: a contiguous head dimension and 16-byte aligned rows
  if (a.step_k_head_size != 1 || a.step_v_head_size != 1 || a.step_k_sl % 8 != 0 || a.step_v_sl % 8 != 0 || a.step_k_head_num % 8 != 0 ||
      a.step_v_head_num % 8 != 0 || (reinterpret_cast<uintptr_t>(a.K) & 15) != 0 || (reinterpret_cast<uintptr_t>(a.V) & 15) != 0)
    return refuse("attention, query blocks over a paged cache: K / V rows must be contiguous in the head dimension and 16-byte aligned");
  AttnSplitParams& sp = pl.pp.sp;
  AttnParams& p = sp.a;
  p.q = a.Q;
  p.k = reinterpret_cast<const _Float16*>(a.K);
  p.v = reinterpret_cast<const _Float16*>(a.V);
  p.dst = a.dst;
  p.dst16 = static_cast<_Float16*>(const_cast<void*>(dst16));
  p.qk_scale = a.QK_scale * a.Q_sc * a.K_sc;
  p.out_scale = a.V_sc / a.dst_sc;
  p.flags = a.attn_flags;
  p.head_num = a.head_num, p.heads_kv = a.heads_kv, p.head_size = a.head_size, p.sl_q = a.sl_q, p.sl_kv = a.sl_kv;
  p.step_q_head_num = a.step_q_head_num, p.step_q_sl = a.step_q_sl;  // (packed rows: no batch step of Q or dst)
  p.step_k_head_num = a.step_k_head_num, p.step_k_sl = a.step_k_sl, p.step_k_head_size = 1;
  p.step_v_head_num = a.step_v_head_num, p.step_v_sl = a.step_v_sl, p.step_v_head_size = 1;
  p.step_dst_head_num = a.step_dst_head_num, p.step_dst_sl = a.step_dst_sl;
  p.hs_pad = a.head_size;
  size_t slot_blocks;
  block_paged_ranges(kn, a.batch_size, a.heads_kv, a.head_num / a.heads_kv, a.sl_q, a.sl_kv, &slot_blocks, &sp.nsplit, &sp.keys_per_split);
  sp.g_full = a.head_num / a.heads_kv;
  sp.kmove = kv_lens, sp.kdelta = kv_len_bias;
  sp.dyn_min_keys = kn.dyn_ranges ? std::max(1, kn.block_min_keys) : 0;
  pl.pp.pg = page, pl.pp.q_start = q_start;
  pl.hs_pad = p.hs_pad;
  pl.grid = dim3(unsigned(slot_blocks * a.heads_kv), unsigned(sp.nsplit), unsigned(a.batch_size));
  pl.block = dim3(256);
  pl.merge_grid = dim3(unsigned(a.head_num), unsigned(a.sl_q), unsigned(a.batch_size));
  pl.partial_bytes = size_t(a.batch_size) * a.sl_q * a.head_num * sp.nsplit * (2 + a.head_size) * 4;
  pl.ok = true;
  return pl;
}

// ---- prompt-sized query blocks over a paged cache (ns_hip_attn_prefill_paged) ------------------------------------------------------------------------
// One launch of the 128-row kernel's PAGED instantiation for every call the entry serves: there is no other kernel to give a call to, so one row is a
// plan like any other.  The instantiation: the padded head size, SB for a biased call and for a score scale that is not positive (SB scales the
// scores up front; the unbiased instantiations take the maximum of RAW scores), PAD for a head size that is not 64 / 128 / 256.
AttnPrefillPagedPlan attn_prefill_paged_plan(const attn_fp32_fp16_fp16_fp32_fwd_args_t& a, const void* dst16, const AttnKnobs& kn, const AttnPage& page,
                                             const int* q_start, const int* kv_lens, int kv_len_bias, std::string* why) {
  AttnPrefillPagedPlan pl;
  memset(&pl.pp, 0, sizeof(pl.pp));
  auto refuse = [&](const char* text) {
    *why = text;
    return pl;
  };
  if (a.Q_layout != ATTN_FWD_LAYOUT_PLAIN || a.K_layout != ATTN_FWD_LAYOUT_PLAIN || a.V_layout != ATTN_FWD_LAYOUT_PLAIN ||
      a.dst_layout != ATTN_FWD_LAYOUT_PLAIN)
    return refuse("attention: only ATTN_FWD_LAYOUT_PLAIN tensors are supported");
  if (!q_start) return refuse("attention, prompt blocks over a paged cache: dQStart is null");
  if (!kv_lens) return refuse("attention, prompt blocks over a paged cache: dKvLens is null");
  if (a.batch_size < 1) return refuse("attention, prompt blocks over a paged cache: batch_size (the requests) must be at least 1");
  if (a.head_size < 8 || a.head_size % 8 != 0 || a.head_size > 256)
    return refuse("attention, prompt blocks over a paged cache: head_size must be a multiple of 8, at most 256");
  // (the head-size-256 PAGED instantiations of the 128-row kernel need scratch with the whole register file: not built — docs/open_items.md)
  if (a.head_size > 128)
    return refuse("attention, prompt blocks over a paged cache: head sizes above 128 are not served (the 256-wide kernel would spill registers)");
  if (a.heads_kv < 1 || a.head_num < 1 || a.head_num % a.heads_kv != 0)
    return refuse("attention, prompt blocks over a paged cache: head_num must be a multiple of heads_kv");
  if (a.sl_q < 1) return refuse("attention, prompt blocks over a paged cache: sl_q is max_q, the most query rows of one request (at least 1)");
  if (a.sl_kv < 1) return refuse("attention, prompt blocks over a paged cache: sl_kv is the capacity of a request (at least 1 key)");
  if (const char* text = attn_page_refusal(a, page)) return refuse(text);
  if (a.step_k_head_size != 1 || a.step_v_head_size != 1 || a.step_k_sl % 8 != 0 || a.step_v_sl % 8 != 0 || a.step_k_head_num % 8 != 0 ||
      a.step_v_head_num % 8 != 0 || (reinterpret_cast<uintptr_t>(a.K) & 15) != 0 || (reinterpret_cast<uintptr_t>(a.V) & 15) != 0)
    return refuse("attention, prompt blocks over a paged cache: K / V rows must be contiguous in the head dimension and 16-byte aligned");
  const size_t nqb = (size_t(a.sl_q) + 127) / 128, wgs = nqb * size_t(a.head_num) * size_t(a.batch_size);
  if (wgs >= (size_t(1) << 31))
    return refuse("attention, prompt blocks over a paged cache: ceil(max_q / 128) * head_num * batch_size must stay below 2^31 workgroups");
  AttnParams& p = pl.pp.a;
  p.q = a.Q;
  p.k = reinterpret_cast<const _Float16*>(a.K);
  p.v = reinterpret_cast<const _Float16*>(a.V);
  p.dst = a.dst;
  p.dst16 = static_cast<_Float16*>(const_cast<void*>(dst16));
  p.qk_scale = a.QK_scale * a.Q_sc * a.K_sc;
  p.out_scale = a.V_sc / a.dst_sc;
  p.flags = a.attn_flags;
  p.head_num = a.head_num, p.heads_kv = a.heads_kv, p.head_size = a.head_size, p.sl_q = a.sl_q, p.sl_kv = a.sl_kv;
  p.step_q_head_num = a.step_q_head_num, p.step_q_sl = a.step_q_sl;  // (packed rows: no batch step of Q or dst; the pools: none of K or V)
  p.step_k_head_num = a.step_k_head_num, p.step_k_sl = a.step_k_sl, p.step_k_head_size = 1;
  p.step_v_head_num = a.step_v_head_num, p.step_v_sl = a.step_v_sl, p.step_v_head_size = 1;
  p.step_dst_head_num = a.step_dst_head_num, p.step_dst_sl = a.step_dst_sl;
  p.hs_pad = a.head_size <= 64 ? 64 : 128;
  // the slopes, as attn_plan sets them
  const int all_heads = kn.alibi_heads > 0 ? kn.alibi_heads : a.head_num;
  p.alibi_head_off = kn.alibi_heads > 0 ? kn.alibi_off : 0;
  if ((a.attn_flags & NS_ATTN_FLAG_IS_ALIBI8) && (p.alibi_head_off < 0 || p.alibi_head_off + a.head_num > all_heads))
    return refuse("attention: head partition (ns_hip_attn_set_head_partition) does not contain this call's heads");
  const int lf = 1 << int(floor(log2(double(all_heads))));
  p.alibi_log2_floor = lf;
  p.alibi_m0 = powf(2.0f, -8.f / float(lf));
  p.alibi_m1 = powf(2.0f, -4.f / float(lf));
  const bool biased = (a.attn_flags & (NS_ATTN_FLAG_IS_ALIBI8 | NS_ATTN_FLAG_IS_TANH30)) != 0;
  pl.pp.pg = page, pl.pp.q_start = q_start, pl.pp.kv_lens = kv_lens, pl.pp.kdelta = kv_len_bias;
  pl.hs_pad = p.hs_pad;
  pl.sb = biased || !(p.qk_scale > 0.f);
  pl.pad = a.head_size != p.hs_pad;
  pl.nqb = int(nqb);
  pl.grid = dim3(unsigned(wgs));
  pl.block = dim3(256);
  pl.lds = size_t(2) * (pl.hs_pad == 64 ? a2_stage_bytes<64>() : a2_stage_bytes<128>());
  pl.aligned = (reinterpret_cast<uintptr_t>(a.dst) & 15) == 0 && a.step_dst_sl % 4 == 0 && a.step_dst_head_num % 4 == 0 &&
               (!dst16 || (reinterpret_cast<uintptr_t>(dst16) & 7) == 0);
  // the remap is a bijection of the workgroup ids whatever a workgroup then does, so the ones that leave early do not disturb it, and the query
  // blocks that stay still share their kv head's pages through one XCD's L2: the rule attn_plan uses, requests in the place of the batch
  pl.xcd_map = !kn.no_xcd_map && (size_t(a.heads_kv) * a.batch_size) % 8 == 0;
  pl.ok = true;
  return pl;
}

}  // namespace ns
