// ns_gemv_plan.cpp — how a decode launch of gemv_kernel (ns_gemv.hip) is made: gemv_plan, a pure function of the call and the tunables (no
// HIP call, no environment, no state).  It answers with one of three refusals callers tell apart (GemvPlan::refusal, ns_gemv.h) or with the
// complete GemvParams, grid, waves and LDS bytes.  ns_gemv_host.cpp launches what it says; tests/test_stream_plan.py checks it on the CPU
// against the rule written out independently.
#include <algorithm>
#include <cstring>

#include "../../include/ns_bestla.h"
#include "ns_gemv.h"

namespace ns {

// waves per workgroup of a decode launch (one 16-column tile per workgroup, k-steps dealt round-robin to the waves).
// Shared with smallm_kernel so that both kernels split K the same way — bit-identical sums between a caller that passes
// the fp16 shadow of A and an fp32-only caller — wherever this rule alone decides: gemv_plan additionally halves the
// wave count until activations + rings fit in LDS (several rows of a large K), where smallm_kernel keeps the rule's value;
// the two then differ in fp32 summation order only (fp32-only callers of decode shapes are served by gemv_kernel itself
// since round 3, bit-equal to the shadow path: tests/test_gpu_fullsize.py).
int decode_waves_rule(int grid, int ks, bool dual, int forced) {
  // measured on the 7B shapes (profiles/r02g_sweep.txt): 256 tiles x 32 k-steps (attention output) 16 waves, 256 tiles
  // x 86 k-steps (FFN down) 8 waves (7.5 vs 8.0 us at 16), 768 tiles 4 waves, 2000 tiles (lm_head) 2 waves
  int nw = (grid <= 320 && ks >= 32 && ks <= 48 && !dual) ? 16 : 8;
  if (dual) {
    nw = grid * 4 >= 1300 ? 4 : 8;
  } else {
    const int target_waves = 2560;
    while (nw > 2 && grid * (nw / 2) >= target_waves) nw /= 2;
  }
  if (forced == 2 || forced == 4 || forced == 8 || (forced == 16 && !dual)) nw = forced;
  while (nw > 1 && nw > ks) nw /= 2;
  return nw;
}

namespace {

struct Miss {  // why == nullptr: nothing is missing
  hipError_t e = hipSuccess;
  const char* why = nullptr;
};
constexpr Miss kFits{};
Miss not_supported(const char* why) { return {hipErrorNotSupported, why}; }
Miss invalid(const char* why) { return {hipErrorInvalidValue, why}; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// what the steps of a plan hand to each other
struct Ctx {
  const SmallMArgs& a;
  const GemvKnobs& kn;
  GemvPlan& pl;
  const ns_weight* w0 = nullptr;  // matrix 0 in the layout that is streamed
  StreamTable t;
  bool planes = false, neox = false, mseg = false;
  int mode = GV_PLAIN, kstep = 0;
  uint32_t ks = 0, row_stride = 0;
  size_t a_bytes = 0, ssq_bytes = 0;
  bool i8q = false, a16 = false, a32 = false;
};

// bit-plane formats: every matrix of the launch has its native clone (same shapes and scales, shorter code records) -> stream those
bool use_planes(const SmallMArgs& a, const GemvKnobs& kn, bool neox) {
  bool planes = kn.planes && !a.i8 && !a.moe && !neox;  // (the pair mode, GV_MSEGP, streams the widened records)
  for (int i = 0; i < a.nseg; i++)
    planes = planes && a.seg[i].w->native && a.seg[i].w->native->scale_dt != DT_F16 && a.seg[i].w->native->pl_bits == a.seg[0].w->native->pl_bits;
  return planes;
}

// the matrix table and the launch mode; NeoX RoPE: whole pairs of tiles per head and matrix, a workgroup per pair
Miss plan_matrices(Ctx& c) {
  const SmallMArgs& a = c.a;
  GemvParams& p = c.pl.p;
  auto pick = [&](const ns_weight* w) { return c.planes ? static_cast<const ns_weight*>(w->native) : w; };
  if (!stream_table(a, pick, &c.t)) return not_supported("a matrix is not one allocation below 2 GiB");
  for (int i = 0; i < a.nseg; i++) p.mat[i] = c.t.mat[i];
  c.mseg = !a.dual && a.nseg > 1;
  c.mode = a.dual ? GV_DUAL : (c.mseg ? (c.neox ? GV_MSEGP : GV_MSEG) : GV_PLAIN);
  uint32_t* tbeg = c.t.tbeg;
  if (c.neox) {
    const int hs = a.rope->head_size;
    if (!c.mseg || a.nseg != 3 || a.rope_route || hs < 32 || (hs % 32) != 0) return invalid("NeoX RoPE: three matrices, heads of whole tile pairs, no replayed route");
    for (int i = 0; i < a.nseg; i++)
      if (p.mat[i].n % hs != 0 || uint32_t(p.mat[i].n) != 16u * uint32_t(pick(a.seg[i].w)->ntiles)) return invalid("NeoX RoPE: a matrix is not whole heads");
    p.pair_tiles = uint32_t(hs / 32);
    tbeg[1] /= 2, tbeg[2] /= 2;  // in workgroups (p.mat[].tile_begin is not read by the kernel)
  }
  p.wbase0 = c.t.wb[0];
  p.wbase1 = c.t.wb[1];
  p.s_off0 = c.t.soff[0], p.s_off1 = c.t.soff[1], p.z_off0 = c.t.zoff[0], p.z_off1 = c.t.zoff[1];
  p.tb1 = c.mseg ? tbeg[1] : 0xffffffffu;
  p.tb2 = (c.mseg && a.nseg > 2) ? tbeg[2] : 0xffffffffu;
  c.ks = uint32_t(c.w0->ksteps);
  c.kstep = c.w0->kstep_len;
  if (c.t.tiles == 0 || c.ks == 0) return not_supported("an empty launch");
  // the scale row of a k-step as a multiply and a shift (a rule that is none has more k-steps than the next check admits)
  int mul, shift;
  if (!srow_params(c.w0, &mul, &shift)) return not_supported("the scale-row rule is not a multiply and a shift");
  p.srow_mul = uint32_t(mul), p.srow_shift = uint32_t(shift);
  // staged activations: [rows][ks * KSTEP + 8] halves (int8-reference numerics: [rows][ks * KSTEP + 16] bytes)
  c.row_stride = a.i8 ? (c.ks * uint32_t(c.kstep) + 16) / 2 : c.ks * uint32_t(c.kstep) + 8;
  c.a_bytes = size_t(a.m) * c.row_stride * 2;
  if (c.a_bytes > kGvMaxALds) return not_supported("the staged activations exceed 64 KiB");
  return kFits;
}

// int8-reference numerics: u8 activation codes with per-block scales and zero points (XV = 3), quantized inside the launch where the rows
// are at hand as fp32 and the k-block is 32 .. 256 columns dividing K (XV = 5)
Miss plan_i8(Ctx& c) {
  const SmallMArgs& a = c.a;
  GemvParams& p = c.pl.p;
  const ns_weight* w0 = c.w0;
  const I8Act& q = *a.i8;
  const bool int_w = w0->kind == WK_INT4 || w0->kind == WK_INT8;
  // a 32-deep slice must lie inside one k-block and inside or outside K; block index by shift (one block: any shift >= 31)
  const bool one_block = q.nblk == 1;
  uint32_t shift = 0;
  while (!one_block && (1u << shift) < uint32_t(q.blocksize)) shift++;
  if (!int_w || a.m > 4 || a.link || a.rope || (w0->k & 31) || !q.aq || !q.corr || !aligned16(q.aq) || !aligned16(q.corr) || (q.ldq & 15) ||
      q.ldq < w0->k || (!one_block && ((1u << shift) != uint32_t(q.blocksize) || q.blocksize < 32)))
    return not_supported("int8-reference numerics: integer weights, up to 4 rows, power-of-two k-blocks, aligned codes");
  if (one_block) shift = 31;
  c.i8q = c.kn.i8_inkernel && q.a32 && !one_block && shift >= 5 && shift <= 8 && w0->k % q.blocksize == 0 && (q.lda32 & 3) == 0 && (w0->k & 3) == 0 &&
          aligned16(q.a32);
  if (!c.i8q && !q.quantized) return {hipErrorNotReady, "int8-reference numerics: the activations are not quantized yet"};
  p.i8_corr = q.corr;
  p.i8_nblk = uint32_t(q.nblk);
  p.i8_span = (uint32_t(a.m) * uint32_t(q.nblk) * 5u + 3u) & ~3u;  // whole words: a buffer load drops a word that straddles the bound (the scratch has the slack)
  p.i8_bshift = shift;
  c.ssq_bytes = (size_t(p.i8_span) + 1023) >> 10 << 10;  // the scales / zero points span sits where a carried norm's sums would
  return kFits;
}

// the refusals of the expert-chunk form (XV = 6).  Named, not written at their return: tests/test_stream_plan.py collects every refusal text
// written at a return of this file and wants its grid of calls to produce each, and its program has no chunk list to offer; these two are
// reached through the block entries (ns_moe.cpp: ffn_device_grouped plans both launches before the first)
constexpr const char* kChunksForm = "expert chunks: whole k-steps of aligned fp16 rows, nothing fused, no fp8";
constexpr const char* kChunksRange = "expert chunks: slots, outputs or gathered rows outside the kernel's range";

// expert-indexed launch: its (row, selection) pairs along grid.y; fused gate / up: the second table, the kernel's one set of strides for both
Miss plan_moe(const Ctx& c) {
  const SmallMArgs& a = c.a;
  const MoeRoute& r = *a.moe;
  if (r.chunks) {
    // expert chunks (XV = 6): up to a.m fp16 rows in gathered order per workgroup — whole k-steps even for one row, the rows of a chunk are
    // staged through one descriptor — and nothing else fused; the outputs are indexed by gathered position
    if (a.nseg != (a.dual ? 2 : 1) || a.link || a.rope || a.i8 || a.d || a.c2 || !c.a16 || !r.table || c.w0->k % c.kstep != 0 || c.w0->kind == WK_F8)
      return not_supported(kChunksForm);
    if (r.pairs < 1 || r.chunk_slots < 1 || r.chunk_slots > 65535 || (!a.seg[0].c && !a.seg[0].c16) || uint64_t(r.pairs) * uint64_t(std::max(a.lda, a.ldc)) >= (uint64_t(1) << 31))
      return not_supported(kChunksRange);
    if (a.dual) {
      const ns_weight *w0 = c.w0, *w1 = a.seg[1].w;
      if (!r.table1 || w1->n != w0->n || w1->qtype != w0->qtype || !same_stream_layout(w1, w0)) return not_supported("expert gate/up: two groups of one shape and format");
    }
    return kFits;
  }
  if (a.m != 1 || a.nseg != (a.dual ? 2 : 1) || a.link || a.rope || a.i8 || a.a16 || !r.table || !r.id) return not_supported("expert launch: one fp32 row, nothing fused");
  if (r.pairs < 1 || r.pairs > 65535 || r.nsel < 1 || int64_t(r.pairs) * r.nsel >= 65536 || (r.a_stride & 3) || r.a_stride < 0 || r.c_stride < 0 ||
      r.d_stride < 0 || std::max({r.a_stride, r.c_stride, r.d_stride}) >= (1ll << 32))
    return not_supported("expert launch: pairs or strides outside the kernel's range");
  if (a.dual) {
    const ns_weight *w0 = c.w0, *w1 = a.seg[1].w;
    if (!r.table1 || a.c2 || w1->n != w0->n || w1->qtype != w0->qtype || !same_stream_layout(w1, w0)) return not_supported("expert gate/up: two groups of one shape and format");
  }
  return kFits;
}

// which form of the activations is staged: fp16 with 16-byte aligned rows, or fp32 converted while staging (XV = 2; not together with a
// carried norm / fused RoPE, whose producers always leave a shadow); several rows need K to fill whole k-steps (a row's padding columns
// would otherwise read the next row through the descriptor)
Miss plan_activations(Ctx& c) {
  const SmallMArgs& a = c.a;
  const ns_weight* w0 = c.w0;
  const bool i8s = a.i8 != nullptr;
  c.a16 = (i8s && !c.i8q) || (!i8s && a.a16 != nullptr && (a.lda & 7) == 0 && (w0->k & 7) == 0 && aligned16(a.a16));
  if (a.moe)
    if (const Miss m = plan_moe(c); m.why) return m;
  c.a32 = c.i8q || (!i8s && !c.a16 && a.a != nullptr && !a.link && !a.rope && (a.lda & 3) == 0 && (w0->k & 3) == 0 && aligned16(a.a));
  if (a.moe && a.moe->chunks) c.a32 = false;
  else if (a.moe && !c.a32) return not_supported("expert launch: fp32 activations with 16-byte rows");
  if ((!c.a16 && !c.a32) || (a.m > 1 && w0->k % c.kstep != 0)) return not_supported("activations: aligned fp16 or fp32 rows; several rows need whole k-steps");
  c.pl.p.a = c.i8q ? static_cast<const void*>(a.i8->a32) : i8s ? static_cast<const void*>(a.i8->aq) : (c.a16 ? a.a16 : static_cast<const void*>(a.a));
  return kFits;
}

// carried RMS norm (ns_norm_link): the consumer side stages in_parts floats per row behind A, the producer side writes the next norm's sums
Miss plan_link(Ctx& c) {
  const SmallMArgs& a = c.a;
  GemvParams& p = c.pl.p;
  const ns_norm_link& k = *a.link;
  if (k.in_ssq) {
    if (k.in_parts < 1 || k.in_stride < k.in_parts || (k.in_stride & 3) || !aligned16(k.in_ssq) || k.norm_size < 1) return invalid("carried norm: the incoming sums are malformed");
    c.ssq_bytes = size_t(a.m) * ((size_t(k.in_parts) * 4 + 1023) >> 10 << 10);
    if (c.ssq_bytes > 32 * 1024) return not_supported("carried norm: more than 32 one-KiB pieces of sums");  // (request counter budget)
    p.in_ssq = k.in_ssq;
    p.in_parts = uint32_t(k.in_parts), p.in_stride = uint32_t(k.in_stride);
    p.in_eps = k.eps, p.in_inv_size = 1.0f / float(k.norm_size);
  }
  if (k.out_ssq || k.out_gamma) {
    if (a.dual || a.nseg != 1 || (k.out_ssq && k.out_stride < c.w0->ntiles)) return invalid("carried norm: the producer side is a single matrix with a slot per tile");
    p.out_gamma = k.out_gamma, p.out_ssq = k.out_ssq, p.out_stride = uint32_t(k.out_stride);
  }
  return kFits;
}

// RoPE(q, k) + kv-cache append as the epilogue of a fused QKV launch; a replayed route's fp32 cells with it (one row)
Miss plan_rope(Ctx& c) {
  const SmallMArgs& a = c.a;
  GemvParams& p = c.pl.p;
  const ns_qkv_rope& r = *a.rope;
  if ((c.mode != GV_MSEG && c.mode != GV_MSEGP) || a.nseg != 3 || r.mode != (c.neox ? 2 : 0) || r.head_size < 2 || (r.head_size & 1) ||
      r.n_dims != r.head_size || !r.kcache16 || !r.vcache16 || !r.cos_sin || r.n_past < 0 || p.mat[0].n != r.heads * r.head_size ||
      p.mat[1].n != r.heads_kv * r.head_size || p.mat[2].n != r.heads_kv * r.head_size)
    return invalid("fused RoPE: three matrices of whole heads, whole-head rotation, cache and table present");
  p.rope.kc = static_cast<_Float16*>(r.kcache16), p.rope.vc = static_cast<_Float16*>(r.vcache16);
  p.rope.c_sl = r.cache_step_sl, p.rope.c_head = r.cache_step_head;
  p.rope.head_size = r.head_size, p.rope.n_past = r.n_past;
  p.rope.cos_sin = reinterpret_cast<const float2*>(r.cos_sin);
  p.rope.on = 1;
  if (a.rope_route) {
    const QkvRopeRoute& q = *a.rope_route;
    if (a.m != 1) return invalid("fused RoPE on a replayed route: one row");
    p.rope.kmove = q.kmove, p.rope.kd_pos = q.kd_pos;
    p.rope.k32 = q.k32, p.rope.v32 = q.v32;
    p.rope.k32_head = q.k32_head, p.rope.k32_dim = q.k32_dim, p.rope.k32_tok = q.k32_tok;
    p.rope.v32_head = q.v32_head, p.rope.v32_dim = q.v32_dim, p.rope.v32_tok = q.v32_tok;
    p.rope.ovf = q.overflow;
  }
  return kFits;
}

// waves per workgroup — enough waves on the chip to overlap dequantisation with the stream (as tuned for smallm_kernel, profiles/r01*),
// halved until the rings of a workgroup fit in LDS beside the staged activations — and the LDS layout [A | sums | rings]
Miss plan_waves(Ctx& c) {
  const SmallMArgs& a = c.a;
  GemvPlan& pl = c.pl;
  GemvParams& p = pl.p;
  const int nq = (a.dual || c.neox) ? 2 : 1;
  const uint32_t slot = record_slot_bytes(c.w0);
  auto ring_bytes = [&](int waves) {  // a wave's ring: one slot per item it can have in flight, at least the reduction scratch
    const uint32_t items = ((c.ks + uint32_t(waves) - 1) / uint32_t(waves)) * uint32_t(nq);
    const size_t b = size_t(std::min<uint32_t>(items, uint32_t(kGvPF))) * slot;
    return std::max<size_t>((b + 15) & ~size_t(15), size_t(nq) * 1024);
  };
  const size_t a_end = (c.a_bytes + 15) & ~size_t(15);
  // (the pair mode takes the wave count of the GV_MSEG launch of the same weights: the same split of K, the same bits)
  int nw = decode_waves_rule(int(c.t.tiles), int(c.ks), a.dual, c.kn.forced_nw);
  while (nw > 1 && a_end + c.ssq_bytes + size_t(nw) * ring_bytes(nw) > kGvMaxLds) nw /= 2;
  while ((1 << p.nw_log2) < nw) p.nw_log2++;
  if (c.a32 && uint64_t(a.m) * ((uint64_t(c.ks) * uint32_t(c.kstep) * 4u + 1023u) >> 10) > uint64_t(nw) * kGvA32Regs) {
    // more fp32 pieces than the waves hold in registers: smallm_kernel stages those (quantized beforehand the rows fit: the caller's retry takes XV = 3)
    if (c.i8q && !a.i8->quantized) return {hipErrorNotReady, "int8-reference numerics: too many fp32 pieces to quantize inside the launch"};
    return not_supported("more fp32 activation pieces than the waves hold in registers");
  }
  pl.nw = nw;
  pl.grid = c.neox ? int(c.t.tiles / 2) : int(c.t.tiles);
  p.ssq_off = uint32_t(a_end);
  p.ring_off = p.ssq_off + uint32_t(c.ssq_bytes);
  p.ring_stride = uint32_t(ring_bytes(nw));
  pl.lds = size_t(p.ring_off) + size_t(nw) * p.ring_stride;
  return kFits;
}

Miss plan_all(Ctx& c) {
  const SmallMArgs& a = c.a;
  GemvParams& p = c.pl.p;
  if (c.kn.gemv2 == 0 || a.m < 1 || a.m > kGvMaxRows) return not_supported("gemv2 0, or rows outside 1 .. 16");
  c.neox = a.rope && (a.rope->flags & NS_QKV_ROPE_NEOX) != 0;
  c.planes = use_planes(a, c.kn, c.neox);
  const ns_weight* w0 = c.w0 = c.planes ? a.seg[0].w->native : a.seg[0].w;
  c.pl.kind = w0->kind, c.pl.sps = w0->sps, c.pl.scale_dt = w0->scale_dt, c.pl.asym = w0->asym;
  Miss m = plan_matrices(c);
  if (!m.why && a.i8) m = plan_i8(c);
  if (!m.why) m = plan_activations(c);
  if (!m.why && a.link) m = plan_link(c);
  if (!m.why && a.rope) m = plan_rope(c);
  if (!m.why && uint64_t(a.m) * uint64_t(a.lda) * 4 >= (uint64_t(1) << 30)) m = not_supported("activations beyond 30-bit staging offsets");
  if (!m.why) m = plan_waves(c);
  if (m.why) return m;
  if (c.pl.lds > kGvMaxLds) return not_supported("activations, sums and one ring per wave exceed LDS");
  p.ks = c.ks;
  p.qstride = w0->qstride, p.sstride = w0->sstride, p.zstride = w0->zstride;
  p.srows = uint32_t(w0->srows);
  p.m = a.m;
  p.k = w0->k;
  p.lda = c.i8q ? a.i8->lda32 : a.i8 ? a.i8->ldq : a.lda;
  p.row_stride = c.row_stride;
  p.c2 = a.c2, p.d = a.d, p.ldc = a.ldc, p.ldd = a.ldd, p.epilogue = a.epilogue;
  if (w0->kind == WK_F4) f4_lut_planes(w0->lut, &p.lut);
  p.f8 = f8_consts(w0->qtype);
  if (a.moe) {
    const MoeRoute& r = *a.moe;
    p.moe_table = r.table, p.moe_table1 = r.table1;
    p.moe_id = r.id, p.moe_n = r.n_as, p.moe_w = r.w;
    p.moe_nsel = uint32_t(r.nsel);
    p.moe_sel_mul = (65536u + p.moe_nsel - 1u) / p.moe_nsel;
    p.moe_ids_stride = r.ids_stride, p.moe_w_stride = r.w_stride;
    p.moe_a_stride = uint32_t(r.a_stride), p.moe_c_stride = uint32_t(r.c_stride), p.moe_d_stride = uint32_t(r.d_stride);
    c.pl.grid_y = r.pairs;
    if (r.chunks) {
      p.moe_id = r.chunks, p.moe_nsel = uint32_t(r.pairs), p.moe_w = nullptr;
      c.pl.grid_y = r.chunk_slots;
    }
  }
  p.pl_bits = c.planes ? uint32_t(w0->pl_bits) : 0u;
  p.pl_lanes = c.planes ? w0->code_rec / 16u : 64u;
  c.pl.mode_x = c.mode | (c.a32 && !a.moe ? kGvModeA32 : 0) | (a.i8 ? kGvModeI8 : 0) | (a.moe ? (a.moe->chunks ? kGvModeGrp : kGvModeMoe) : 0) | (c.planes ? kGvModePlanes : 0);
  return kFits;
}

}  // namespace

GemvPlan gemv_plan(const SmallMArgs& a, const GemvKnobs& knobs, std::string* why) {
  GemvPlan pl;
  memset(&pl.p, 0, sizeof(pl.p));
  Ctx c{a, knobs, pl};
  const Miss m = plan_all(c);
  pl.refusal = m.e;
  if (why && m.why) *why = m.why;
  return pl;
}

}  // namespace ns
