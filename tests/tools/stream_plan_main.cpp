// Program of tests/test_stream_plan.py: prints the plans gemvs_plan (neural-speed_amd/csrc/ns_gemvs_plan.cpp) and gemv_plan (ns_gemv_plan.cpp)
// make for a fixed grid of decode calls, one line each:  <the call, key=value> | <every field of the plan, key=value> why=<text>.
// Host code only: no HIP call is made, no tensor exists — the pointers are made-up addresses.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "ns_gemvs.h"
#include "ns_gemm_plan.cpp"
#include "ns_gemv_plan.cpp"
#include "ns_gemvs_plan.cpp"

using namespace ns;

template <class T>
static T* at(uintptr_t a) {
  return reinterpret_cast<T*>(a);
}

// formats: 0 int4 sps 4 bf16 symmetric, 1 int4 sps 1 fp32 asymmetric, 2 int8 sps 2 bf16, 3 f4 (nf4) sps 2 fp16, 4 fp8 sps 2 fp32;
// 5 .. 7: format 0 with a native bit-plane clone of 3 bits (5), whose scales are fp16 (6), whose second matrix has 2 bits (7).
// One allocation per matrix (index i): codes at its base, scales behind them, zero points behind those.
struct Weight {
  ns_weight w, native;
};
static void make_weight(int fmt, int n, int k, int i, Weight* out, int grp = 0) {
  ns_weight& w = out->w;
  const int f = fmt >= 5 ? 0 : fmt;
  const int kinds[] = {WK_INT4, WK_INT4, WK_INT8, WK_F4, WK_F8}, spss[] = {4, 1, 2, 2, 2};
  const uint32_t sdts[] = {DT_BF16, DT_F32, DT_BF16, DT_F16, DT_F32}, qts[] = {DT_S4, DT_S4, DT_S8, DT_F4_NF4, DT_F8_E4M3};
  w.kind = kinds[f], w.sps = spss[f], w.scale_dt = sdts[f], w.qtype = qts[f], w.asym = f == 1;
  w.n = n, w.k = k;
  w.kstep_len = kind_is_8bit(w.kind) ? 64 : 128;
  w.ksteps = (k + w.kstep_len - 1) / w.kstep_len, w.ntiles = (n + 15) / 16;
  w.blocksize = w.kstep_len / w.sps, w.srows = w.ksteps;
  // grp: a group of whole k-steps (grp columns), or one group over K (-1) — one scale per record, a scale row per group (three arrays)
  if (grp) w.sps = 1, w.blocksize = grp < 0 ? (k + w.kstep_len - 1) / w.kstep_len * w.kstep_len : grp, w.srows = grp < 0 ? 1 : (k + grp - 1) / grp;
  const uint32_t sbytes = w.sps * (w.scale_dt == DT_F32 ? 4 : 2);
  w.qstride = 1024, w.sstride = 16 * sbytes, w.zstride = w.asym ? 16 * w.sps : 0;
  w.codes_bytes = size_t(w.ntiles) * w.ksteps * 1024, w.scales_bytes = size_t(w.ntiles) * w.srows * w.sstride, w.zps_bytes = size_t(w.ntiles) * w.srows * w.zstride;
  const uintptr_t base = uintptr_t(0x100000000) * (i + 1);
  w.codes = at<uint4>(base), w.scales = at<void>(base + w.codes_bytes);
  w.zps = w.asym ? at<int8_t>(base + w.codes_bytes + w.scales_bytes) : nullptr;
  w.alloc_bytes = w.codes_bytes + w.scales_bytes + w.zps_bytes, w.single_span = true;
  for (int e = 0; e < 16; e++) w.lut[e] = (_Float16)float(e - 8), w.lutf[e] = float(e - 8);
  if (fmt >= 5) {  // the clone: records of code_rec bytes with the scales behind them in one stream
    ns_weight& c = out->native;
    c = w;
    c.pl_bits = fmt == 7 && i == 1 ? 2 : 3;
    c.code_rec = 256u * c.pl_bits;
    if (fmt == 6) c.scale_dt = DT_F16;
    c.qstride = c.sstride = c.code_rec + 16 * sbytes;
    c.codes_bytes = size_t(c.ntiles) * c.ksteps * c.qstride, c.scales_bytes = 0;
    c.codes = at<uint4>(base + 0x80000000), c.scales = at<void>(base + 0x80000000 + c.code_rec);
    c.alloc_bytes = c.codes_bytes, c.native = nullptr;
    w.native = &c;
  }
}

// one layout field of a fused launch's second matrix changed (0: none; 12: its tile count, which matters to gate/up pairs only)
static void mismatch(ns_weight* w, int mis) {
  switch (mis) {
    case 1: w->kind = w->kind == WK_INT4 ? WK_F4 : WK_INT4; break;
    case 2: w->sps = w->sps == 2 ? 1 : 2; break;
    case 3: w->scale_dt = w->scale_dt == DT_F16 ? DT_BF16 : DT_F16; break;
    case 4: w->asym = !w->asym; break;
    case 5: w->k += 128; break;
    case 6: w->ksteps++; break;
    case 7: w->qstride += 64; break;
    case 8: w->sstride += 16; break;
    case 9: w->zstride += 16; break;
    case 10: w->srows++; break;
    case 11: w->blocksize *= 2; break;
    case 12: w->n += 16, w->ntiles++; break;
    case 13: w->qtype ^= 1u << 16; break;  // (gemv_plan's expert gate/up pairs compare these two as well)
    case 14: w->n += 1; break;
    default: break;
  }
}

struct Case {
  int fmt = 0, m = 8, n = 4096, k = 4096;
  int form = 0;  // 0 single, 1 gate/up, 2 / 3 fused QKV of that many matrices (nkv: columns of k and v, 0 = as q)
  int nkv = 0;
  int act = 1;   // 0 fp32 only, 1 fp32 + aligned fp16 shadow, 2 shadow 8 bytes off, 3 shadow with lda % 8 != 0, 4 none, 5 fp32 with lda % 4 != 0,
                 // 6 a leading dimension of 2^24
  int mis = 0;
  int grp = 0;   // the weights' group in columns where it is above one k-step (-1: per-channel); 0: the format's own
  int spec = 0;  // 1 a scale-row rule that is no multiply-and-shift, 2 a weight of several spans, 3 an allocation of 2 GiB, 4 no columns,
                 // 5 a gate/up pair of three matrices
  int feat = 0;  // gemvs: 1 carried norm, 2 fused RoPE, 3 int8-reference numerics, 4 expert launch (presence only)
  // gemv_plan: carried norm 1 consumer, 2 producer, 3 both, 4 consumer stride < parts, 5 producer stride < tiles, 6 consumer of 3000 parts,
  // 7 consumer of 1536 parts
  int link = 0;
  // fused RoPE: 1 mode 0, 2 NeoX; hs head size; rbrk 1 replayed route, 2 n_dims != head_size, 3 mode mismatch, 4 q one tile wider
  int rope = 0, hs = 128, rbrk = 0;
  // int8-reference numerics: i8 1 on; nblk 0 = K / i8bs blocks; i8q 1 = quantized; i8a 1 = fp32 rows at hand
  int i8 = 0, i8bs = 128, nblk = 0, i8q = 1, i8a = 1;
  // expert launch: moe 1 on; mbrk 1 no table1 on a pair, 2 a_stride % 4 != 0
  int moe = 0, pairs = 1, nsel = 1, mbrk = 0;
  // knobs of gemvs_plan / gemv_plan
  int gvs = 1, sl = 0, wv = 0, gr = 0, tb = -1, fin = 1, dma = 1, cus = 256;
  int gemv2 = 1, planes = 1, fnw = 0, i8k = 1;
};

static void print_case(const char* fn, const Case& c) {
  printf("fn=%s fmt=%d grp=%d m=%d n=%d k=%d form=%d nkv=%d act=%d mis=%d spec=%d feat=%d link=%d rope=%d hs=%d rbrk=%d i8=%d i8bs=%d nblk=%d i8q=%d i8a=%d moe=%d pairs=%d "
         "nsel=%d mbrk=%d gvs=%d sl=%d wv=%d gr=%d tb=%d fin=%d dma=%d cus=%d gemv2=%d planes=%d fnw=%d i8k=%d | ",
         fn, c.fmt, c.grp, c.m, c.n, c.k, c.form, c.nkv, c.act, c.mis, c.spec, c.feat, c.link, c.rope, c.hs, c.rbrk, c.i8, c.i8bs, c.nblk, c.i8q, c.i8a, c.moe, c.pairs,
         c.nsel, c.mbrk, c.gvs, c.sl, c.wv, c.gr, c.tb, c.fin, c.dma, c.cus, c.gemv2, c.planes, c.fnw, c.i8k);
}

// the call both plans are asked about; the structs it points to
struct Call {
  Weight w[3];
  SmallMArgs a{};
  ns_norm_link link;
  ns_qkv_rope rope;
  QkvRopeRoute route;
  I8Act i8;
  MoeRoute moe;
};
static void make_call(const Case& c, Call* out) {
  Call& x = *out;
  const int nseg = c.form == 0 ? 1 : c.form == 1 ? 2 : c.form;
  const int nq = c.rope && c.rbrk == 4 ? c.n + 16 : c.n, nk = c.form >= 2 && c.nkv ? c.nkv : c.n;
  make_weight(c.fmt, c.spec == 4 ? 0 : nq, c.k, 0, &x.w[0], c.grp);
  make_weight(c.fmt, nk, c.k, 1, &x.w[1], c.grp);
  make_weight(c.fmt, nk, c.k, 2, &x.w[2], c.grp);
  mismatch(&x.w[1].w, c.mis);
  if (c.spec == 1)  // one scale row per 1000 k-steps: (s * 1049) >> 20 is s / 1000 up to k-step 2998 only
    for (Weight& w : x.w) w.w.blocksize = 1000 * w.w.kstep_len, w.w.srows = (w.w.ksteps + 999) / 1000;
  if (c.spec == 2) x.w[nseg - 1].w.single_span = false;
  if (c.spec == 3) x.w[nseg - 1].w.alloc_bytes = size_t(1) << 31;
  SmallMArgs& a = x.a;
  a.m = c.m, a.ldc = nq, a.nseg = nseg, a.epilogue = c.form == 1 ? NS_EPI_SILU : NS_EPI_ADD;
  a.lda = c.act == 3 ? c.k + 4 : c.act == 5 ? c.k + 2 : c.act == 6 ? 1 << 24 : c.k;
  a.a = c.act == 4 ? nullptr : at<const float>(0x10000000);
  a.a16 = c.act >= 1 && c.act <= 3 ? at<const void>(uintptr_t(0x20000000) + (c.act == 2 ? 8 : 0)) : nullptr;
  if (c.form != 1) a.d = at<const float>(0x60000000), a.ldd = nq + 32;
  for (int i = 0; i < nseg; i++) {
    a.seg[i].w = &x.w[i].w;
    a.seg[i].c = at<float>(0x30000000 + 0x1000000 * uintptr_t(i));
    a.seg[i].c16 = i == 0 ? at<void>(0x40000000) : nullptr;
  }
  a.dual = c.form == 1;
  if (c.spec == 5) a.nseg = 3, a.seg[2].w = &x.w[2].w, a.seg[2].c = nullptr, a.seg[2].c16 = nullptr;
  if (a.dual && !c.moe) a.c2 = at<float>(0x50000000);
  memset(&x.link, 0, sizeof(x.link));
  if (c.link || c.feat == 1) {
    ns_norm_link& l = x.link;
    if (c.link != 2 && c.link != 5) l.in_ssq = at<const float>(0x70000000), l.in_parts = c.link == 6 ? 3000 : c.link == 7 ? 1536 : 256, l.in_stride = c.link == 4 ? 252 : l.in_parts + 4;
    if (c.link == 2 || c.link == 3 || c.link == 5) l.out_gamma = at<const float>(0x71000000), l.out_ssq = at<float>(0x72000000), l.out_stride = (nq + 15) / 16 - (c.link == 5);
    l.eps = 1e-5f, l.norm_size = c.k;
    a.link = &l;
  }
  memset(&x.rope, 0, sizeof(x.rope));
  if (c.rope || c.feat == 2) {
    ns_qkv_rope& r = x.rope;
    r.flags = c.rope == 2 ? NS_QKV_ROPE_NEOX : 0, r.mode = (c.rope == 2) != (c.rbrk == 3) ? 2 : 0;
    r.head_size = c.hs, r.n_dims = c.rbrk == 2 ? c.hs / 2 : c.hs, r.heads = c.n / c.hs, r.heads_kv = nk / c.hs, r.n_past = 7;
    r.kcache16 = at<void>(0x78000000), r.vcache16 = at<void>(0x79000000), r.cos_sin = at<const float>(0x7a000000);
    r.cache_step_sl = c.hs, r.cache_step_head = 4096LL * c.hs;
    a.rope = &r;
    if (c.rbrk == 1) {
      memset(&x.route, 0, sizeof(x.route));
      x.route.k32 = at<float>(0x7b000000), x.route.v32 = at<float>(0x7c000000), x.route.kd_pos = 3;
      a.rope_route = &x.route;
    }
  }
  if (c.i8 || c.feat == 3) {
    I8Act& q = x.i8;
    q = I8Act{};
    q.nblk = c.nblk ? c.nblk : (c.k + c.i8bs - 1) / c.i8bs, q.blocksize = c.i8bs;
    q.aq = at<const uint8_t>(0x80000000), q.ldq = (c.k + 15) & ~15, q.corr = at<const uint8_t>(0x81000000);
    q.a32 = c.i8a ? at<const float>(0x10000000) : nullptr, q.lda32 = c.k, q.rows = c.m, q.cols = c.k, q.quantized = c.i8q != 0;
    a.i8 = &q;
  }
  if (c.moe || c.feat == 4) {
    MoeRoute& r = x.moe;
    r = MoeRoute{};
    r.table = at<const MoeExpertRow>(0x90000000), r.id = at<const int32_t>(0x91000000), r.n_as = 8;
    r.table1 = a.dual && c.mbrk != 1 ? at<const MoeExpertRow>(0x92000000) : nullptr;
    r.pairs = c.pairs, r.nsel = c.nsel, r.ids_stride = c.nsel, r.w = at<const float>(0x93000000), r.w_stride = c.nsel;
    r.a_stride = c.mbrk == 2 ? c.k + 2 : c.k, r.c_stride = c.n, r.d_stride = c.n + 32;
    a.moe = &r;
  }
}

static const char* err_name(hipError_t e) {
  return e == hipSuccess ? "OK" : e == hipErrorNotSupported ? "NOTSUP" : e == hipErrorNotReady ? "NOTREADY" : e == hipErrorInvalidValue ? "INVAL" : "OTHER";
}
template <class Mat>
static void print_mats(const Mat* mat) {
  for (int i = 0; i < 3; i++) printf("mn%d=%d mtb%d=%u mc%d=%d mc16_%d=%d ", i, mat[i].n, i, mat[i].tile_begin, i, mat[i].c != nullptr, i, mat[i].c16 != nullptr);
}

static void run_gemvs(const Case& c) {
  Call x;
  make_call(c, &x);
  GvsKnobs kn;
  kn.gvs = c.gvs, kn.gvs_slices = c.sl, kn.gvs_waves = c.wv, kn.gvs_grid = c.gr, kn.gvs_table = c.tb, kn.gvs_finalize = c.fin, kn.table_dma = c.dma != 0;
  std::string why = "-";
  const GvsPlan pl = gemvs_plan(x.a, kn, c.cus, &why);
  const GvsParams& p = pl.p;
  const GvsFinParams& f = pl.f;
  print_case("gemvs", c);
  if (pl.refusal != hipSuccess) {
    printf("err=%s why=%s\n", err_name(pl.refusal), why.c_str());
    return;
  }
  printf("err=OK kind=%d sps=%d sdt=%u asym=%d mode=%d grid=%d nwaves=%d lds=%zu convert=%d cvt_bytes=%zu slab_bytes=%zu tickets=%d tblimg=%d cost=%.17g ", pl.kind,
         pl.sps, pl.scale_dt, int(pl.asym), pl.mode, pl.grid, pl.nwaves, pl.lds, int(pl.convert), pl.cvt_bytes, pl.slab_bytes, int(pl.want_tickets),
         int(pl.want_table_image), pl.cost);
  printf("so=%u,%u,%u zo=%u,%u,%u wb=%d,%d,%d a=%d ks=%u ksl=%u slog=%u qstride=%u sstride=%u zstride=%u srows=%u smul=%u sshift=%u tb1=%u tb2=%u ntiles=%u tg=%u "
         "tbase=%u trem=%u ns=%u pm=%d pk=%d lda=%d rstride=%u ctl=%u red=%u ring=%u rings=%u redw=%u reds=%u aoff=%u abytes=%u lut0=%u lut7=%u owned=%d ",
         p.so0, p.so1, p.so2, p.zo0, p.zo1, p.zo2, p.wb0 != nullptr, p.wb1 != nullptr, p.wb2 != nullptr, p.a != nullptr, p.ks, p.ksl, p.s_log2, p.qstride, p.sstride,
         p.zstride, p.srows, p.srow_mul, p.srow_shift, p.tb1, p.tb2, p.ntiles, p.tg_count, p.tiles_base, p.tiles_rem, p.ns, p.m, p.k, p.lda, p.row_stride, p.ctl_off,
         p.red_off, p.ring_off, p.ring_stride, p.red_wave, p.red_slot, p.a_off, p.a_bytes, p.lut16[0], p.lut16[7],
         (p.slab != nullptr) + (p.tickets != nullptr) + (p.tbl_img != nullptr) + (f.slab != nullptr));
  print_mats(p.mat);
  printf("c2=%d d=%d ldc=%d ldd=%d epi=%d pslab=%u f8=%u fs=%u fnt=%u fnq=%u ftb1=%u ftb2=%u fm=%d fn=%d,%d,%d fc2=%d fd=%d fldc=%d fldd=%d fepi=%d why=%s\n",
         p.c2 != nullptr, p.d != nullptr, p.ldc, p.ldd, p.epilogue, p.slab_bytes, p.f8.c2, f.slices, f.ntiles, f.nq, f.tb1, f.tb2, f.m, f.mat[0].n, f.mat[1].n,
         f.mat[2].n, f.c2 != nullptr, f.d != nullptr, f.ldc, f.ldd, f.epilogue, why.c_str());
}

static void run_gemv(const Case& c) {
  Call x;
  make_call(c, &x);
  GemvKnobs kn;
  kn.gemv2 = c.gemv2, kn.planes = c.planes != 0, kn.forced_nw = c.fnw, kn.i8_inkernel = c.i8k != 0;
  std::string why = "-";
  const GemvPlan pl = gemv_plan(x.a, kn, &why);
  const GemvParams& p = pl.p;
  print_case("gemv", c);
  if (pl.refusal != hipSuccess) {
    printf("err=%s why=%s\n", err_name(pl.refusal), why.c_str());
    return;
  }
  // which of the call's arrays the kernel stages: 1 the fp16 shadow, 2 the fp32 rows, 3 the u8 codes, 4 the int8 call's fp32 rows
  const int asrc = p.a == x.a.a16 && x.a.a16 ? 1 : x.a.i8 && p.a == x.a.i8->aq ? 3 : x.a.i8 && p.a == x.a.i8->a32 ? 4 : p.a == x.a.a ? 2 : 0;
  printf("err=OK kind=%d sps=%d sdt=%u asym=%d modex=%d grid=%d gridy=%d nw=%d lds=%zu asrc=%d ks=%u qstride=%u nwlog=%u so=%u,%u zo=%u,%u sstride=%u zstride=%u "
         "srows=%u smul=%u sshift=%u tb1=%u tb2=%u pm=%d pk=%d lda=%d rstride=%u ssq=%u ring=%u rings=%u ",
         pl.kind, pl.sps, pl.scale_dt, int(pl.asym), pl.mode_x, pl.grid, pl.grid_y, pl.nw, pl.lds, asrc, p.ks, p.qstride, p.nw_log2, p.s_off0, p.s_off1, p.z_off0,
         p.z_off1, p.sstride, p.zstride, p.srows, p.srow_mul, p.srow_shift, p.tb1, p.tb2, p.m, p.k, p.lda, p.row_stride, p.ssq_off, p.ring_off, p.ring_stride);
  printf("i8corr=%d i8span=%u i8nblk=%u i8shift=%u moet=%d moet1=%d moen=%d moew=%d msel=%u mmul=%u mids=%d mws=%d mas=%u mcs=%u mds=%u plbits=%u pllanes=%u "
         "pairt=%u ",
         p.i8_corr != nullptr, p.i8_span, p.i8_nblk, p.i8_bshift, p.moe_table != nullptr, p.moe_table1 != nullptr, p.moe_n, p.moe_w != nullptr, p.moe_nsel,
         p.moe_sel_mul, p.moe_ids_stride, p.moe_w_stride, p.moe_a_stride, p.moe_c_stride, p.moe_d_stride, p.pl_bits, p.pl_lanes, p.pair_tiles);
  print_mats(p.mat);
  printf("c2=%d d=%d ldc=%d ldd=%d epi=%d inssq=%d inparts=%u instride=%u ininv=%.9g ogamma=%d ossq=%d ostride=%u oovf=%d ron=%d rhs=%d rnp=%d rkd=%d rk32=%d "
         "f8=%u lut0=%u why=%s\n",
         p.c2 != nullptr, p.d != nullptr, p.ldc, p.ldd, p.epilogue, p.in_ssq != nullptr, p.in_parts, p.in_stride, double(p.in_inv_size), p.out_gamma != nullptr,
         p.out_ssq != nullptr, p.out_stride, p.out_ovf != nullptr, p.rope.on, p.rope.head_size, p.rope.n_past, p.rope.kd_pos, p.rope.k32 != nullptr, p.f8.c2,
         p.lut.lo[0], why.c_str());
}

static void gemvs_grid() {
  const int rows[] = {1, 2, 3, 4, 5, 8, 9, 12, 16, 17};
  // n x k; 4160: no multiple of the 4-bit k-step; 4100: k % 8 != 0
  const int shapes[][2] = {{16, 128},    {272, 2048},   {1024, 4096},  {4096, 4096}, {4096, 11008}, {4096, 14336}, {11008, 4096}, {14336, 4096},
                           {32000, 4096}, {128, 8192},  {8192, 1024},  {4096, 4160}, {4096, 4100}};
  // forms: single, gate/up, QKV of two, QKV of three with 1024 kv columns, a ragged n (n + 4 columns)
  struct Form {
    int form, nkv, dn;
  };
  const Form forms[] = {{0, 0, 0}, {1, 0, 0}, {2, 0, 0}, {3, 1024, 0}, {0, 0, 4}};
  // 1. every format, row count, shape and form at three device sizes, by shape (the default) and pinned from one row
  for (int fmt = 0; fmt < 5; fmt++)
    for (int m : rows)
      for (const auto& s : shapes)
        for (const Form& f : forms)
          for (int cus : {64, 256, 304})
            for (int gvs : {1, 2}) {
              if (gvs == 2 && cus != 256) continue;
              Case c;
              c.fmt = fmt, c.m = m, c.n = s[0] + f.dn, c.k = s[1], c.form = f.form, c.nkv = f.nkv, c.cus = cus, c.gvs = gvs;
              run_gemvs(c);
            }
  // 2. activations
  for (int fmt : {0, 3})
    for (int m : {1, 2, 8, 16})
      for (const auto& s : {shapes[1], shapes[3], shapes[5], shapes[11]})
        for (int act = 0; act <= 4; act++)
          for (int form : {0, 1}) {
            Case c;
            c.fmt = fmt, c.m = m, c.n = s[0], c.k = s[1], c.act = act, c.form = form, c.gvs = 2;
            run_gemvs(c);
          }
  // 3. the second matrix differs; the other kernel's features; the special weights
  for (int fmt : {0, 1, 3})
    for (int mis = 1; mis <= 12; mis++)
      for (int form : {1, 2, 3}) {
        Case c;
        c.fmt = fmt, c.form = form, c.mis = mis, c.gvs = 3;
        run_gemvs(c);
      }
  for (int feat = 1; feat <= 4; feat++) {
    Case c;
    c.feat = feat, c.form = feat == 2 ? 3 : 0, c.gvs = 3;
    run_gemvs(c);
  }
  {
    Case c;
    c.spec = 5, c.form = 1, c.gvs = 3;
    run_gemvs(c);
  }
  for (int spec = 1; spec <= 4; spec++)
    for (int form : {0, 3}) {
      Case c;
      c.spec = spec, c.form = form, c.gvs = 2, c.m = spec == 1 ? 1 : 8;
      if (spec == 1) c.fmt = 1, c.k = 3200 * 128, c.n = 16;
      run_gemvs(c);
    }
  // 4. knobs
  const int kshapes[][2] = {{16, 128}, {4096, 4096}, {4096, 14336}, {14336, 4096}, {128, 8192}, {32000, 4096}};
  for (int fmt = 0; fmt < 5; fmt++)
    for (int m : {1, 2, 5, 8, 16})
      for (const auto& s : kshapes)
        for (int form : {0, 1, 3}) {
          Case b;
          b.fmt = fmt, b.m = m, b.n = s[0], b.k = s[1], b.form = form, b.nkv = form == 3 ? 1024 : 0, b.gvs = 3;
          for (int gvs = 0; gvs <= 3; gvs++) {
            Case c = b;
            c.gvs = gvs;
            run_gemvs(c);
          }
          for (int sl : {1, 2, 3, 8, 32, 64})
            for (int fin : {0, 1}) {
              Case c = b;
              c.sl = sl, c.fin = fin;
              run_gemvs(c);
            }
          for (int wv : {1, 7, 15, 16, 20}) {
            Case c = b;
            c.wv = wv;
            run_gemvs(c);
          }
          for (int gr : {2, 16, 64, 512}) {
            Case c = b;
            c.gr = gr;
            run_gemvs(c);
          }
          for (int tb : {-1, 0, 1})
            for (int dma : {0, 1}) {
              Case c = b;
              c.tb = tb, c.dma = dma;
              run_gemvs(c);
            }
        }
  // 5. the split-K slab at 2 GiB (gate/up pairs of 524288 columns in 32 slices) and just below; more tile units than tickets
  for (int n : {524288, 524272}) {
    Case c;
    c.form = 1, c.n = n, c.sl = 32, c.gvs = 3;
    run_gemvs(c);
  }
  for (int n : {65536 * 16, 65537 * 16}) {
    Case c;
    c.fmt = 2, c.n = n, c.k = 128, c.sl = 2, c.fin = 0, c.gvs = 3;
    run_gemvs(c);
  }
}

static void gemv_grid() {
  const int rows[] = {1, 2, 4, 5, 16, 17};
  // 1. every format and row count: square, long K, 2048 deep (16 rows exceed the staging limit, 15 do not), the lm_head
  for (int fmt = 0; fmt < 8; fmt++)
    for (int m : {1, 2, 4, 5, 7, 15, 16, 17})
      for (const auto& s : {std::pair<int, int>{4096, 4096}, {4096, 11008}, {11008, 4096}, {4096, 2048}, {32000, 4096}, {4100, 4100}})
        for (int form : {0, 1, 2, 3})
          for (int act : {0, 1}) {
            if (form >= 1 && s.first == 32000) continue;
            Case c;
            c.fmt = fmt, c.m = m, c.n = s.first, c.k = s.second, c.form = form, c.nkv = form == 3 ? 1024 : 0, c.act = act;
            run_gemv(c);
          }
  for (int act = 0; act <= 6; act++)
    for (int m : {1, 4, 16}) {
      Case c;
      c.m = m, c.act = act, c.k = act == 6 ? 1024 : 4096;
      run_gemv(c);
    }
  for (int spec = 1; spec <= 4; spec++)
    for (int form : {0, 3}) {
      Case c;
      c.spec = spec, c.form = form, c.m = 1;
      if (spec == 1) c.fmt = 1, c.k = 3200 * 128, c.n = 16;
      run_gemv(c);
    }
  // 2. carried norm
  for (int fmt : {0, 1, 5})
    for (int m : {1, 2, 4, 7, 12})
      for (int link = 1; link <= 6; link++)
        for (int form : {0, 1, 3})
          for (int act : {0, 1}) {
            Case c;
            c.fmt = fmt, c.m = m, c.link = link, c.form = form, c.nkv = form == 3 ? 1024 : 0, c.act = act;
            run_gemv(c);
          }
  // (the largest footprint real operands reach: 4096 x 6144 at 5 rows of 1536 partial sums beside 16 rings)
  for (int m : {4, 5}) {
    Case c;
    c.m = m, c.k = 6144, c.link = 7;
    run_gemv(c);
  }
  // 3. fused RoPE
  for (int fmt : {0, 3, 5})
    for (int m : {1, 2, 16})
      for (int rope : {1, 2})
        for (int hs : {64, 128, 48, 2})
          for (int rbrk = 0; rbrk <= 4; rbrk++)
            for (int form : {3, 2, 0}) {
              if (form != 3 && (rbrk || hs != 128)) continue;
              Case c;
              c.fmt = fmt, c.m = m, c.rope = rope, c.hs = hs, c.rbrk = rbrk, c.form = form;
              c.n = hs == 48 ? 4032 : 4096, c.nkv = hs == 48 ? 1008 : 1024;
              for (int link : {0, 1}) {
                c.link = link;
                run_gemv(c);
              }
            }
  // 4. int8-reference numerics
  for (int fmt : {0, 1, 2, 3})
    for (int m : {1, 4, 5})
      for (int bs : {4096, 32, 128, 512, 48, 16})
        for (int i8q : {0, 1})
          for (int i8a : {0, 1})
            for (int i8k : {0, 1})
              for (const auto& s : {std::pair<int, int>{4096, 4096}, {11008, 4096}}) {
                Case c;
                c.fmt = fmt, c.m = m, c.i8 = 1, c.i8bs = bs, c.i8q = i8q, c.i8a = i8a, c.i8k = i8k, c.n = s.first, c.k = s.second, c.act = 0;
                run_gemv(c);
              }
  // (a made-up block count: the scales' span pushes the rings out of LDS — at 6000 blocks until 4 waves are left, at 30000 for good)
  for (int nblk : {30000, 6000})
    for (int feat : {0, 1, 2}) {
      Case c;
      c.m = 4, c.i8 = 1, c.i8a = 0, c.nblk = nblk, c.act = 0, c.link = feat == 1, c.rope = feat == 2, c.form = feat == 2 ? 3 : 0;
      run_gemv(c);
    }
  // 5. expert launches
  for (int fmt : {0, 1, 3, 4})
    for (int form : {0, 1})
      for (const auto& pn : {std::pair<int, int>{1, 1}, {65535, 1}, {21845, 3}, {16384, 4}, {65536, 1}, {0, 1}, {4, 2}})
        for (int mbrk = 0; mbrk <= 2; mbrk++)
          for (int mis : {0, 13, 14, 5})
            for (int act : {0, 1, 5}) {
              if ((mis && (form == 0 || mbrk)) || (act && (mis || mbrk))) continue;
              Case c;
              c.fmt = fmt, c.m = 1, c.form = form, c.moe = 1, c.pairs = pn.first, c.nsel = pn.second, c.mbrk = mbrk, c.mis = mis, c.act = act, c.n = 14336;
              run_gemv(c);
            }
  for (int m : {2}) {
    Case c;
    c.m = m, c.moe = 1, c.act = 0;
    run_gemv(c);
  }
  // 6. fp32 rows in more pieces than the waves hold (11008 columns: 4 waves): plain, and the int8 call quantizing in the launch
  for (int m : rows)
    for (int i8 : {0, 1})
      for (int i8q : {0, 1}) {
        Case c;
        c.m = m, c.n = 11008, c.act = 0, c.i8 = i8, c.i8q = i8q;
        run_gemv(c);
      }
  // 7. knobs
  for (int fmt : {0, 2, 5})
    for (int m : {1, 4, 16})
      for (const auto& s : {std::pair<int, int>{4096, 4096}, {4096, 1024}, {32000, 4096}, {16, 128}})
        for (int form : {0, 1}) {
          Case b;
          b.fmt = fmt, b.m = m, b.n = s.first, b.k = s.second, b.form = form;
          Case c = b;
          c.gemv2 = 0;
          run_gemv(c);
          c = b, c.planes = 0;
          run_gemv(c);
          for (int fnw : {2, 4, 8, 16, 3}) {
            c = b, c.fnw = fnw;
            run_gemv(c);
          }
        }
}

// the group-size ladder of tests/test_gpu_group_sizes.py at its own shapes (263 columns; K = 1920, 2048, 1952): what each pinned call of that
// module is planned as.  4-bit records (formats 0, 1, 3): groups 128, 256, 384, 512, 640, per-channel; 8-bit and fp8 records (2, 4): 64, 128, 192,
// 320, per-channel
static void ladder_grid() {
  for (int fmt = 0; fmt < 5; fmt++)
    for (int gi = 0; gi < 6; gi++) {
      const bool b8 = fmt == 2 || fmt == 4;
      const int g4[] = {128, 256, 384, 512, 640, -1}, g8[] = {64, 128, 192, 320, -1, 0};
      const int grp = b8 ? g8[gi] : g4[gi];
      if (!grp) continue;
      for (int k : {1920, 2048, 1952}) {
        Case b;
        b.fmt = fmt, b.grp = grp, b.n = 263, b.k = k;
        // gemv_kernel: rows x shadow / fp32 only x forced waves; the fused launches; the int8-reference variant (k-block = the group)
        for (int m : {1, 4, 8, 16})
          for (int act : {0, 1})
            for (int fnw : {0, 2, 16})
              for (int form : {0, 1, 3}) {
                if ((fnw && (m != 1 || form)) || (form && m != 1 && m != 8)) continue;
                Case c = b;
                c.m = m, c.act = act, c.fnw = fnw, c.form = form;
                run_gemv(c);
              }
        for (int m : {1, 3})
          for (int i8q : {0, 1}) {
            if (fmt >= 3) continue;
            Case c = b;
            c.m = m, c.act = 0, c.i8 = 1, c.i8bs = grp < 0 ? k : grp, c.i8q = i8q;
            run_gemv(c);
          }
        // gemvs_kernel pinned ("gvs" 3): rows x forced slices x forced streaming waves, finished in the launch and by the finalize launch
        for (int m : {2, 8, 16})
          for (int sl : {0, 1, 2, 4, 8})
            for (int wv : {0, 3, 7})
              for (int fin : {0, 1}) {
                if ((sl == 0) != (wv == 0) || (sl == 0 && m != 8)) continue;
                Case c = b;
                c.m = m, c.gvs = 3, c.sl = sl, c.wv = wv, c.fin = fin;
                run_gemvs(c);
              }
      }
    }
}

int main() {
  gemvs_grid();
  gemv_grid();
  ladder_grid();
  return 0;
}
