// ns_gemm_plan.cpp — which kernel serves a prefill GEMM, in which tile form, over which grid: gemm_plan, a pure function of the call and the
// tunables (no HIP call, no environment, no state), plus the scale-row rule every matrix launcher shares.  ns_gemm.cpp launches what it says;
// tests/test_gemm_plan.py checks it on the CPU against the rule written out independently.
#include <cstring>

#include "ns_gemm.h"
#include "ns_launch.h"

namespace ns {

void srow_rule(const ns_weight* w, int* num, int* den) {
  if (w->blocksize >= w->k) {
    *num = 0;
    *den = 1;
  } else if (w->sps > 1 || w->blocksize == w->kstep_len) {
    *num = 1;
    *den = 1;
  } else {
    *num = w->kstep_len;
    *den = w->blocksize;
  }
}

bool srow_params(const ns_weight* w0, int* mul, int* shift) {
  int num, den;
  srow_rule(w0, &num, &den);
  if (num == 0) {
    *mul = 0;
    *shift = 0;
  } else if (num == den) {
    *mul = 1;
    *shift = 0;
  } else {
    const int ratio = den / num;
    if ((ratio & (ratio - 1)) == 0) {
      *mul = 1;
      *shift = __builtin_ctz(ratio);
    } else {
      *shift = 20;
      *mul = ((1 << 20) + ratio - 1) / ratio;
      for (int s = 0; s < w0->ksteps; s++)
        if (((s * *mul) >> 20) != s / ratio) return false;
    }
  }
  return true;
}

// fp8 weights span 2^-15 .. 2^15 per code before their scale: gemm3_kernel takes them when the load found a power of two that keeps every
// scaled code inside fp16 (ns_weights.cpp set_gemm_scale_range) and the "g3_f8" switch is on
bool gemm3_takes(const ns_weight* w, const GemmKnobs& knobs) {
  return w && (w->kind != WK_F8 || (knobs.g3_f8 && w->g2_ok && w->scale_dt == DT_F32 && !w->asym && w->sps <= 2));
}

static bool aligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

static GemmPlan refuse(hipError_t e, std::string* why, const char* reason) {
  GemmPlan pl;
  pl.refusal = e;
  if (why) *why = reason;
  return pl;
}

// the matrices of a fused launch share one format and one record layout (gate/up pairs: the column count and the array sizes as well)
static bool same_layout(const ns_weight* w, const ns_weight* w0, bool with_n_and_bytes) {
  return w->k == w0->k && w->kind == w0->kind && w->sps == w0->sps && w->scale_dt == w0->scale_dt && w->asym == w0->asym &&
         w->ksteps == w0->ksteps && w->qstride == w0->qstride && w->sstride == w0->sstride && w->zstride == w0->zstride &&
         w->srows == w0->srows && w->qtype == w0->qtype &&
         (!with_n_and_bytes || (w->n == w0->n && w->codes_bytes == w0->codes_bytes && w->scales_bytes == w0->scales_bytes && w->zps_bytes == w0->zps_bytes));
}

// fp16 activations: the caller's shadow when it is usable as is, else one conversion pass into scratch.  nullptr: what is missing
static const char* plan_activations(const SmallMArgs& a, const ns_weight* w0, GemmPlan* pl) {
  Gemm2Params& p = pl->p;
  pl->kpad = p.nchunks * kG2KC;
  const _Float16* a16 = static_cast<const _Float16*>(a.a16);
  if (a16 && (w0->k % kG2KC != 0 || (a.lda & 7) != 0 || !aligned(a16, 15))) a16 = nullptr;
  if (a16) {
    p.a16 = a16;
    p.lda16 = a.lda;
  } else if (!a.a) {
    return "fp16-only activations that cannot be multiplied as they are";  // the caller's general path
  } else {
    pl->convert = true;
    pl->cvt_bytes = size_t(a.m) * pl->kpad * 2;
    p.lda16 = pl->kpad;
  }
  if (size_t(a.m) * size_t(p.lda16) * 2 >= (size_t(1) << 32)) return "activations beyond 32-bit byte offsets";
  return nullptr;
}

static void plan_weight(const SmallMArgs& a, const ns_weight* w0, const GemmKnobs& knobs, Gemm2Params* pp) {
  Gemm2Params& p = *pp;
  p.ksteps = w0->ksteps;
  p.ntiles = w0->ntiles;
  p.codes = w0->codes;
  p.scales = w0->scales;
  p.zps = w0->zps;
  p.codes_bytes = uint32_t(w0->codes_bytes);
  p.scales_bytes = uint32_t(w0->scales_bytes);
  p.zps_bytes = uint32_t(w0->zps_bytes);
  p.qstride = w0->qstride;
  p.sstride = w0->sstride;
  p.zstride = w0->zstride;
  p.c = a.seg[0].c;
  p.c16 = static_cast<_Float16*>(a.seg[0].c16);
  p.ldc = a.ldc;
  p.srows = w0->srows;
  p.epilogue = a.epilogue;
  p.d = a.d;
  p.ldd = a.ldd;
  if (w0->kind == WK_F4) f4_lut_planes(w0->lut, &p.lut);
  p.spre = w0->g2_pre;
  p.spost = w0->g2_post;
  p.diag = knobs.diag;
  p.nbn = (w0->ntiles + kG2Tiles - 1) / kG2Tiles;
  p.ksplit = 1;
  p.cps = p.nchunks;
}

// grid, LDS and the kernel of a gemm3_kernel plan whose tile form and K split are set
static void finish_gemm3(GemmPlan* pl) {
  const Gemm2Params& p = pl->p;
  pl->kernel = GK_GEMM3;
  pl->grid = dim3(unsigned(8 * p.cpx * ((p.m + p.bm3 - 1) / p.bm3)), unsigned(p.ksplit));
  pl->lds = with_format(pl->kind, pl->sps, pl->scale_dt, pl->asym, [&](auto kind_c, auto sps_c, auto sk_c, auto asym_c) {
    return size_t(gemm3_lds(kind_c, sps_c, sk_c, asym_c, p.bm3, p.tall3 != 0).bytes(p.wide != 0));
  });
}

// fused gate/up at GEMM size (round 5): gemm3_kernel only, a column block = 4 tile pairs = 64 output columns
static const char* plan_gateup(const SmallMArgs& a, const GemmKnobs& knobs, GemmPlan* pl) {
  Gemm2Params& p = pl->p;
  const ns_weight *w0 = a.seg[0].w, *w = a.seg[1].w;
  if (a.nseg != 2 || !w || a.m < knobs.g3_min_m || knobs.gemm3 != 1 || a.d || kG3M32) return "gate/up pairs: two matrices on gemm3_kernel, no epilogue operand";
  if (!same_layout(w, w0, true)) return "gate/up pairs: the two matrices differ in shape or format";
  if (!p.c && !p.c16) {
    pl->refusal = hipErrorInvalidValue;
    return "no output";
  }
  p.dual = 1;
  p.codes2 = w->codes, p.scales2 = w->scales, p.zps2 = w->zps;
  p.seg_spre[1] = w->g2_pre, p.seg_spost[1] = w->g2_post;  // (the two matrices' largest scales need not share a binade)
  p.c2 = a.c2;
  p.nbn = (w0->ntiles + 3) / 4;
  p.cpx = (p.nbn + 7) / 8;
  p.wide = 1;
  p.bm3 = a.m <= 64 ? 64 : 128;
  finish_gemm3(pl);
  return nullptr;
}

// RoPE + kv-cache append in the epilogue: plain whole-head RoPE, whole 128-column blocks per matrix, 16-byte fp32 / 8-byte cache stores
static bool plan_rope(const SmallMArgs& a, Gemm2Params* pp) {
  Gemm2Params& p = *pp;
  const ns_qkv_rope& r = *a.rope;
  const bool neox = (r.flags & NS_QKV_ROPE_NEOX) != 0;  // NeoX pairs: the head inside one 128-column block (32 / 64 / 128)
  const bool head_ok = r.mode == (neox ? 2 : 0) && (!neox || (r.head_size >= 32 && 128 % r.head_size == 0)) && r.n_dims == r.head_size &&
                       r.head_size >= 4 && (r.head_size & 3) == 0 && r.n_past >= 0;
  const bool shape_ok = a.nseg == 3 && a.seg[0].w->n == r.heads * r.head_size && a.seg[1].w->n == r.heads_kv * r.head_size &&
                        a.seg[2].w->n == r.heads_kv * r.head_size && a.seg[0].w->n % 128 == 0 && a.seg[1].w->n % 128 == 0 && (a.ldc & 3) == 0;
  const bool cache_ok = r.kcache16 && r.vcache16 && r.cos_sin && (r.cache_step_sl & 3) == 0 && (r.cache_step_head & 3) == 0 &&
                        aligned(r.kcache16, 7) && aligned(r.vcache16, 7) && aligned(r.cos_sin, 15);
  const bool out_ok = a.seg[0].c && aligned(a.seg[0].c, 15) && aligned(a.seg[1].c, 15) && aligned(a.seg[2].c, 15) && !a.seg[0].c16 &&
                      !a.seg[1].c16 && !a.seg[2].c16 && a.epilogue == NS_EPI_NONE;
  if (!(head_ok && shape_ok && cache_ok && out_ok) || kG3M32) return false;
  p.rope_on = neox ? 2 : 1, p.rope_hs = r.head_size, p.rope_npast = r.n_past;
  p.rope_tab = reinterpret_cast<const float2*>(r.cos_sin);
  p.rope_kc = static_cast<_Float16*>(r.kcache16), p.rope_vc = static_cast<_Float16*>(r.vcache16);
  p.rope_csl = r.cache_step_sl, p.rope_chead = r.cache_step_head;
  return true;
}

// fused QKV at GEMM size: gemm3_kernel only, whole column blocks per matrix
static const char* plan_qkv(const SmallMArgs& a, const GemmKnobs& knobs, Gemm2Params* pp) {
  Gemm2Params& p = *pp;
  const ns_weight* w0 = a.seg[0].w;
  if (a.nseg > 3 || a.m < knobs.g3_min_m || knobs.gemm3 != 1) return "fused QKV: up to three matrices on gemm3_kernel";
  p.nseg = a.nseg;
  int bn0 = 0;
  for (int i = 0; i < a.nseg; i++) {
    const ns_weight* w = a.seg[i].w;
    if (!same_layout(w, w0, false)) return "fused QKV: the matrices differ in K or format";
    p.seg_spre[i] = w->g2_pre, p.seg_spost[i] = w->g2_post;
    p.seg_bn0[i] = bn0;
    p.seg_n[i] = w->n;
    p.seg_codes[i] = w->codes, p.seg_scales[i] = w->scales, p.seg_zps[i] = w->zps;
    p.seg_codes_bytes[i] = uint32_t(w->codes_bytes), p.seg_scales_bytes[i] = uint32_t(w->scales_bytes);
    p.seg_zps_bytes[i] = uint32_t(w->zps_bytes);
    p.seg_c[i] = a.seg[i].c;
    p.seg_c16[i] = static_cast<_Float16*>(a.seg[i].c16);
    bn0 += (w->ntiles + kG2Tiles - 1) / kG2Tiles;
  }
  p.nbn = bn0;
  if (a.rope && !plan_rope(a, pp)) return "fused QKV + RoPE: outside the epilogue's envelope";
  return nullptr;
}

// K splits of a launch with `tiles` output tiles: until `target` workgroups are in flight, at least 8 chunks per split, at most 8 splits
static int ksplit_for(int tiles, int nchunks, int target) {
  int ks = 1;
  while (ks < 8 && tiles * ks * 2 <= target && nchunks / (ks * 2) >= 8) ks *= 2;
  return ks;
}

// gemm3_kernel's tile form, epilogue form and K split for a single matrix or a fused QKV.  nullptr, or what is missing
static const char* plan_gemm3(const SmallMArgs& a, const ns_weight* w0, const GemmKnobs& knobs, GemmPlan* pl) {
  Gemm2Params& p = pl->p;
  // 128-row tiles (three workgroups per CU hide each other's barrier / dequantisation / output phases) unless the output has so many tiles
  // that the tall ones' halved A traffic wins (profiles/r02r_gemm3_bm.txt: at 2048 rows equal or better up to 11008 columns, 7 % worse at
  // 32000).  Tall wave tiles (256 x 32, "g3_bm" 257): shape by shape at 2048 rows they gain 2-4 % where a workgroup runs long (11008 x 4096,
  // 4096 x 11008, 32000 x 4096) and lose 14 % on 4096 x 4096 (profiles/r03v_gemm3_tall.txt); in a layer's sequence of GEMMs, steady state,
  // choosing them by that rule gained nothing (986 vs 993 TFLOPS, profiles/r03w_prefill_ab.txt) — not selected automatically.  8-bit
  // codes: the 256-row tile's LDS footprint (81 KiB) leaves one workgroup per CU
  const int bm = knobs.g3_bm;
  const int tall_tiles = p.nbn * ((a.m + 255) / 256);
  p.tall3 = bm == 257 && w0->kind == WK_INT4;
  p.bm3 = p.tall3 ? 256 : bm == 64 || bm == 128 || bm == 256 ? bm : a.m <= 64 ? 64 : (tall_tiles >= 1024 && !kind_is_8bit(w0->kind) ? 256 : 128);
  // outputs: the per-wave epilogue by default; the cross-wave one ("g3_wide" 1) measured 2-8 % SLOWER with both outputs on the 7B shapes at
  // 2048 rows (profiles/r05b_gemm3_epilogue_ab.txt: 4096^2 100.4 vs 92.9 us, 11008 x 4096 208.2 vs 204.8, 4096 x 11008 197.5 vs 191.7) and
  // level with the fp32 output alone — its two extra workgroup barriers per 64-row half cost more than the longer store runs return.  A
  // launch without an fp32 output (fp16 only: the consumer is this library's next GEMM) and the gate / up pairs need it (their per-wave
  // runs would be 16 columns)
  const bool f16_only = !p.c && p.nseg <= 1;
  if (f16_only) {
    if (!p.c16) {
      pl->refusal = hipErrorInvalidValue;
      return "no output";
    }
    if (p.bm3 == 256 && !p.tall3) p.bm3 = 128;
  }
  p.wide = (p.bm3 != 256 || p.tall3) && !kG3M32 && !p.rope_on && (knobs.g3_wide != 0 || f16_only);  // (the RoPE epilogue lives in the per-wave form)
  // few output tiles: split K so that the launch still fills the chip with two workgroups per CU.  A launch with the fp16 output only
  // never splits K: the reduction pass writes fp32
  const int ks = ksplit_for(p.nbn * ((a.m + p.bm3 - 1) / p.bm3), p.nchunks, 512);
  if (ks > 1 && !knobs.no_splitk && !knobs.no_partials && p.nseg <= 1 && p.c) {
    p.ksplit = ks;
    p.cps = ((p.nchunks + ks - 1) / ks + 1) & ~1;  // even: a 128-deep superstep never straddles two splits
    pl->part_bytes = size_t(ks) * a.m * w0->n * 4;
  }
  finish_gemm3(pl);
  return nullptr;
}

// gemm2_kernel: single matrices below "g3_min_m" rows or with NS_GEMM3=0.  It writes the fp32 output unconditionally
static const char* plan_gemm2(const SmallMArgs& a, const ns_weight* w0, const GemmKnobs& knobs, GemmPlan* pl) {
  Gemm2Params& p = pl->p;
  if (p.rope_on || w0->kind == WK_F8) return "the RoPE epilogue and the fp8 conversion are gemm3_kernel's";
  if (!p.c) {
    if (!p.c16) pl->refusal = hipErrorInvalidValue;
    return p.c16 ? "gemm2_kernel has no fp16-only output" : "no output";
  }
  const int nbm = (a.m + kG2BM - 1) / kG2BM;
  // few output tiles (M up to a few hundred rows): split K so that the launch still fills the chip
  const int ks = ksplit_for(p.nbn * nbm, p.nchunks, 256);
  if (ks > 1 && !knobs.no_splitk && !knobs.no_partials) {
    p.ksplit = ks;
    p.cps = (p.nchunks + ks - 1) / ks;
    pl->part_bytes = size_t(ks) * a.m * w0->n * 4;
  }
  pl->kernel = GK_GEMM2;
  pl->grid = dim3(unsigned(8 * p.cpx * nbm), unsigned(p.ksplit));
  pl->lds = size_t(kG2Stages) * kG2StageBytes;
  return nullptr;
}

// Rows: a plain fp8 call (fp32 activations in, fp32 result out, one matrix) of up to 64 rows stays on the kernels that served it before —
// the streaming kernel's and gen 1's exact-scale numerics, 3e-5 — and the forms only this kernel has (fp16-only operands, fused launches)
// start at 17.  Otherwise, and with NS_GEMM3 other than 1, fp8 weights stay on the first-generation kernel, which applies the group scale
// to the fp32 MFMA result
static bool f8_call_ok(const SmallMArgs& a, const GemmKnobs& knobs) {
  for (int i = 0; i < a.nseg; i++)
    if (!a.seg[i].w || a.seg[i].w->kind != WK_F8 || !gemm3_takes(a.seg[i].w, knobs)) return false;
  const bool plain = a.nseg == 1 && !a.dual && !a.rope && a.a && a.seg[0].c;
  return knobs.gemm3 == 1 && !kG3M32 && a.m >= 17 && !(plain && a.m <= 64);
}

GemmPlan gemm_plan(const SmallMArgs& a, const GemmKnobs& knobs, std::string* why) {
  if (knobs.v1) return refuse(hipErrorNotSupported, why, "NS_GEMM_V1");
  const ns_weight* w0 = a.seg[0].w;
  const bool f8 = w0->kind == WK_F8;
  if (f8 && !f8_call_ok(a, knobs)) return refuse(hipErrorNotSupported, why, "fp8 weights: not a call gemm3_kernel takes");
  GemmPlan pl;
  pl.refusal = hipErrorNotSupported;
  pl.kind = w0->kind, pl.sps = w0->sps, pl.scale_dt = w0->scale_dt, pl.asym = w0->asym;
  Gemm2Params& p = pl.p;
  memset(&p, 0, sizeof(p));
  if (f8) p.f8 = f8_consts(w0->qtype);
  p.m = a.m;
  p.k = w0->k;
  p.n = w0->n;
  p.nchunks = (w0->k + kG2KC - 1) / kG2KC;
  const char* miss = plan_activations(a, w0, &pl);
  if (!miss && !srow_params(w0, &p.srow_mul, &p.srow_shift)) miss = "the scale-row rule is not a multiply and a shift";
  if (!miss) {
    plan_weight(a, w0, knobs, &p);
    if (a.dual) {
      miss = plan_gateup(a, knobs, &pl);
    } else {
      if (a.nseg > 1) miss = plan_qkv(a, knobs, &p);
      else if (a.rope) miss = "RoPE epilogue on a single matrix";
      p.cpx = (p.nbn + 7) / 8;
      // third-generation kernel (A by LDS DMA, B dequantised in registers) from "g3_min_m" rows; NS_GEMM3=0 keeps the second generation
      // (diagnostics / A-B runs)
      if (!miss) miss = knobs.gemm3 != 0 && a.m >= knobs.g3_min_m ? plan_gemm3(a, w0, knobs, &pl) : plan_gemm2(a, w0, knobs, &pl);
    }
  }
  if (miss) return refuse(pl.refusal, why, miss);
  pl.refusal = hipSuccess;
  return pl;
}

}  // namespace ns
