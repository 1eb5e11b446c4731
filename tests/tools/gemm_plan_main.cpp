// Program of tests/test_gemm_plan.py: prints the plan gemm_plan (neural-speed_amd/csrc/ns_gemm_plan.cpp) makes for a fixed grid of calls, one line
// each:  <the call, key=value> | <every field of the plan, key=value>.
// Host code only: no HIP call is made, no tensor exists — the pointers are made-up addresses.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "ns_gemm.h"
#include "ns_gemm_plan.cpp"

using namespace ns;

// formats: 0 int4 sps 4 bf16 symmetric, 1 int4 sps 1 fp32 asymmetric, 2 int8 sps 2 bf16, 3 f4 (nf4) sps 2 fp16, 4 fp8 sps 2 fp32 (g2_ok),
// 5 the same with g2_ok off, 6 fp8 with a bf16 scale
static ns_weight make_weight(int fmt, int n, int k) {
  ns_weight w;
  const int kinds[] = {WK_INT4, WK_INT4, WK_INT8, WK_F4, WK_F8, WK_F8, WK_F8}, spss[] = {4, 1, 2, 2, 2, 2, 2};
  const uint32_t sdts[] = {DT_BF16, DT_F32, DT_BF16, DT_F16, DT_F32, DT_F32, DT_BF16}, qts[] = {DT_S4, DT_S4, DT_S8, DT_F4_NF4, DT_F8_E4M3, DT_F8_E4M3, DT_F8_E5M2};
  w.kind = kinds[fmt], w.sps = spss[fmt], w.scale_dt = sdts[fmt], w.qtype = qts[fmt], w.asym = fmt == 1, w.g2_ok = fmt != 5;
  w.n = n, w.k = k;
  w.kstep_len = kind_is_8bit(w.kind) ? 64 : 128;
  w.ksteps = (k + w.kstep_len - 1) / w.kstep_len, w.ntiles = (n + 15) / 16;
  w.blocksize = w.kstep_len / w.sps, w.srows = w.ksteps;
  const uint32_t sbytes = w.sps * (w.scale_dt == DT_F32 ? 4 : 2);
  w.qstride = 1024, w.sstride = 16 * sbytes, w.zstride = w.asym ? 16 * w.sps : 0;
  w.codes_bytes = size_t(w.ntiles) * w.ksteps * 1024, w.scales_bytes = size_t(w.ntiles) * w.srows * w.sstride, w.zps_bytes = size_t(w.ntiles) * w.srows * w.zstride;
  w.codes = reinterpret_cast<uint4*>(uintptr_t(0x1000000)), w.scales = reinterpret_cast<void*>(uintptr_t(0x2000000));
  w.zps = w.asym ? reinterpret_cast<int8_t*>(uintptr_t(0x3000000)) : nullptr;
  for (int i = 0; i < 16; i++) w.lut[i] = (_Float16)float(i - 8), w.lutf[i] = float(i - 8);
  return w;
}

// one layout field of a fused launch's second matrix changed (0: none; 12 .. 15 matter to gate/up pairs only)
static void mismatch(ns_weight* w, int mis) {
  switch (mis) {
    case 1: w->k += 64; break;
    case 2: w->kind = w->kind == WK_INT4 ? WK_F4 : WK_INT4; break;
    case 3: w->sps = w->sps == 2 ? 1 : 2; break;
    case 4: w->scale_dt = w->scale_dt == DT_F16 ? DT_BF16 : DT_F16; break;
    case 5: w->asym = !w->asym; break;
    case 6: w->ksteps++; break;
    case 7: w->qstride += 64; break;
    case 8: w->sstride += 16; break;
    case 9: w->zstride += 16; break;
    case 10: w->srows++; break;
    case 11: w->qtype ^= 1u << 16; break;
    case 12: w->n += 16, w->ntiles++; break;
    case 13: w->codes_bytes += 1024; break;
    case 14: w->scales_bytes += 64; break;
    case 15: w->zps_bytes += 64; break;
    default: break;
  }
}

struct Case {
  int fmt = 0, m = 2048, n = 4096, k = 4096;
  int nkv = 0;   // fused QKV: columns of k and v (0: as q)
  int act = 0;   // 0 fp32 only, 1 fp32 + usable fp16 shadow, 2 shadow misaligned by 8 bytes, 3 shadow with lda % 8 != 0, 4 fp16 shadow only
  int out = 0;   // 0 fp32, 1 both, 2 fp16 only, 3 none
  int form = 0;  // 0 single, 2 / 3 fused QKV of that many matrices, 5 QKV + RoPE, 7 gate/up, 8 RoPE on a single matrix
  int mis = 0, brk = 0, neox = 0, hs = 128;
  const char* knob = "none";
  int kval = 0;
};

static float* f32_at(uintptr_t a) { return reinterpret_cast<float*>(a); }

static void run(const Case& c) {
  const bool rope = c.form == 5 || c.form == 8;
  int nq = c.n, nk = c.nkv ? c.nkv : c.n, nv = nk, hs = c.hs;
  int nseg = c.form == 0 || c.form == 8 ? 1 : c.form == 7 || c.form == 2 ? 2 : 3;
  // the RoPE epilogue's conditions, broken one at a time (tests/test_gemm_plan.py rope_ok lists them by the same numbers)
  if (rope) {
    if (c.brk == 1) nseg = 2;
    if (c.brk == 3) hs = 16;
    if (c.brk == 4) hs = 256;
    if (c.brk == 6) hs = 2;
    if (c.brk == 7) hs = 6, nq = 768, nk = nv = 384;
    if (c.brk == 12) nk *= 2;
    if (c.brk == 29) nv *= 2;
    if (c.brk == 13) nq += 64;
    if (c.brk == 14) nk += 64, nv += 64;
  }
  ns_weight w[3] = {make_weight(c.fmt, nq, c.k), make_weight(c.fmt, c.form == 7 ? nq : nk, c.k), make_weight(c.fmt, nv, c.k)};
  mismatch(&w[1], c.mis);
  SmallMArgs a{};
  a.m = c.m, a.lda = c.act == 3 ? c.k + 4 : c.k, a.ldc = nq, a.nseg = nseg, a.epilogue = NS_EPI_NONE;
  a.a = c.act == 4 ? nullptr : f32_at(0x10000000);
  a.a16 = c.act == 0 ? nullptr : reinterpret_cast<const void*>(uintptr_t(0x20000000) + (c.act == 2 ? 8 : 0));
  for (int i = 0; i < nseg; i++) {
    a.seg[i].w = &w[i];
    a.seg[i].c = c.out == 0 || c.out == 1 ? f32_at(0x30000000 + 0x1000000 * uintptr_t(i)) : nullptr;
    a.seg[i].c16 = c.out == 1 || c.out == 2 ? reinterpret_cast<void*>(uintptr_t(0x40000000) + 0x1000000 * uintptr_t(i)) : nullptr;
  }
  a.dual = c.form == 7;
  if (c.form == 7) {
    a.c2 = f32_at(0x50000000);
    if (c.brk == 1) a.nseg = 3, a.seg[2].w = &w[2];
    if (c.brk == 2) a.d = f32_at(0x60000000), a.ldd = nq, a.epilogue = NS_EPI_ADD;
    if (c.brk == 3) a.seg[1].w = nullptr;
  }
  ns_qkv_rope r;
  memset(&r, 0, sizeof(r));
  if (rope) {
    r.flags = c.neox ? NS_QKV_ROPE_NEOX : 0, r.mode = c.neox ? 2 : 0;
    r.head_size = r.n_dims = hs, r.heads = nq / hs, r.heads_kv = (c.brk == 12 ? nv : nk) / hs, r.n_past = 5;
    r.kcache16 = reinterpret_cast<void*>(uintptr_t(0x70000000)), r.vcache16 = reinterpret_cast<void*>(uintptr_t(0x78000000));
    r.cos_sin = f32_at(0x7c000000);
    r.cache_step_sl = hs, r.cache_step_head = 4096LL * hs;
    switch (c.brk) {
      case 2: r.mode = c.neox ? 0 : 2; break;
      case 5: r.n_dims = hs / 2; break;
      case 8: r.kcache16 = nullptr; break;
      case 9: r.vcache16 = nullptr; break;
      case 10: r.cos_sin = nullptr; break;
      case 11: r.n_past = -1; break;
      case 15: a.ldc += 2; break;
      case 16: r.cache_step_sl += 2; break;
      case 17: r.cache_step_head += 2; break;
      case 18: r.kcache16 = reinterpret_cast<void*>(uintptr_t(0x70000004)); break;
      case 19: r.vcache16 = reinterpret_cast<void*>(uintptr_t(0x78000004)); break;
      case 20: r.cos_sin = f32_at(0x7c000008); break;
      case 21: a.seg[0].c = nullptr; break;
      case 22: a.seg[0].c = f32_at(0x30000008); break;
      case 23: a.seg[1].c = f32_at(0x31000008); break;
      case 24: a.seg[2].c = f32_at(0x32000008); break;
      case 25: a.seg[0].c16 = reinterpret_cast<void*>(uintptr_t(0x40000000)); break;
      case 26: a.seg[1].c16 = reinterpret_cast<void*>(uintptr_t(0x41000000)); break;
      case 27: a.seg[2].c16 = reinterpret_cast<void*>(uintptr_t(0x42000000)); break;
      case 28: a.epilogue = NS_EPI_ADD; break;
      case 30: r.heads++; break;
      case 31: a.seg[1].c = a.seg[2].c = nullptr; break;  // (allowed: k and v may go to the cache alone)
      default: break;
    }
    a.rope = &r;
  }
  GemmKnobs kn;
  const struct {
    const char* name;
    int* field;
  } ints[] = {{"gemm3", &kn.gemm3}, {"g3_min_m", &kn.g3_min_m}, {"g3_bm", &kn.g3_bm}, {"g3_wide", &kn.g3_wide}, {"diag", &kn.diag}};
  for (const auto& e : ints)
    if (!strcmp(c.knob, e.name)) *e.field = c.kval;
  const struct {
    const char* name;
    bool* field;
  } bools[] = {{"v1", &kn.v1}, {"g3_f8", &kn.g3_f8}, {"no_splitk", &kn.no_splitk}, {"no_partials", &kn.no_partials}};
  for (const auto& e : bools)
    if (!strcmp(c.knob, e.name)) *e.field = c.kval != 0;
  std::string why = "-";
  const GemmPlan pl = gemm_plan(a, kn, &why);
  const Gemm2Params& p = pl.p;
  // the shared LDS formula, asked directly with the kernel's template arguments (with_format's rule: fp8 scales are fp32, no sps 4 for 8-bit codes)
  size_t ldsf = 0;
  if (pl.kernel == GK_GEMM3) {
    const int sk = w[0].kind == WK_F8 || w[0].scale_dt == DT_F32 ? SK_F32 : w[0].scale_dt == DT_F16 ? SK_F16 : SK_BF16;
    ldsf = gemm3_lds(w[0].kind, w[0].sps, sk, w[0].asym, p.bm3, p.tall3 != 0).bytes(p.wide != 0);
  }
  const char* kernels[] = {"REFUSED", "GEMM2", "GEMM3"};
  printf("fmt=%d m=%d n=%d k=%d nkv=%d act=%d out=%d form=%d mis=%d brk=%d neox=%d hs=%d knob=%s kval=%d | ", c.fmt, c.m, c.n, c.k, c.nkv, c.act, c.out, c.form,
         c.mis, c.brk, c.neox, c.hs, c.knob, c.kval);
  if (pl.kernel == GK_REFUSED) {
    printf("kernel=REFUSED err=%s why=%s\n", pl.refusal == hipErrorNotSupported ? "NOTSUP" : pl.refusal == hipErrorInvalidValue ? "INVAL" : "OTHER", why.c_str());
    return;
  }
  printf("kernel=%s err=%s bm=%d tall=%d dual=%d wide=%d grid=%u,%u,%u lds=%zu ldsf=%zu convert=%d cvt_bytes=%zu kpad=%d ksplit=%d cps=%d part_bytes=%zu "
         "pm=%d pk=%d pn=%d nchunks=%d lda16=%d a16=%d part=%d ksteps=%d ntiles=%d cbytes=%u sbytes=%u zbytes=%u qstride=%u sstride=%u zstride=%u c=%d c16=%d "
         "ldc=%d srows=%d smul=%d sshift=%d epi=%d d=%d ldd=%d nbn=%d cpx=%d nseg=%d bn0=%d,%d,%d segn=%d,%d,%d rope=%d rhs=%d npast=%d csl=%lld chead=%lld "
         "spre=%g spost=%g f8c=%u diag=%d codes2=%d c2=%d pkind=%d psps=%d pasym=%d why=%s\n",
         kernels[pl.kernel], pl.refusal == hipSuccess ? "OK" : "SET", p.bm3, p.tall3, p.dual, p.wide, pl.grid.x, pl.grid.y, pl.grid.z, pl.lds, ldsf,
         int(pl.convert), pl.cvt_bytes, pl.kpad, p.ksplit, p.cps, pl.part_bytes, p.m, p.k, p.n, p.nchunks, p.lda16, p.a16 != nullptr, p.part != nullptr,
         p.ksteps, p.ntiles, p.codes_bytes, p.scales_bytes, p.zps_bytes, p.qstride, p.sstride, p.zstride, p.c != nullptr, p.c16 != nullptr, p.ldc, p.srows,
         p.srow_mul, p.srow_shift, p.epilogue, p.d != nullptr, p.ldd, p.nbn, p.cpx, p.nseg, p.seg_bn0[0], p.seg_bn0[1], p.seg_bn0[2], p.seg_n[0], p.seg_n[1],
         p.seg_n[2], p.rope_on, p.rope_hs, p.rope_npast, p.rope_csl, p.rope_chead, double(p.spre), double(p.spost), p.f8.c2, p.diag, p.codes2 != nullptr,
         p.c2 != nullptr, pl.kind, pl.sps, int(pl.asym), why.c_str());
}

int main() {
  const int rows[] = {1, 2, 16, 17, 33, 64, 65, 128, 129, 256, 257, 2048, 4096};
  const int shapes[][2] = {{144, 192}, {128, 1024}, {4096, 4096}, {11008, 4096}, {32000, 4096}, {4096, 11008}};  // n x k
  const struct {
    const char* name;
    int value;
  } knobs[] = {{"none", 0}, {"v1", 1}, {"gemm3", 0}, {"gemm3", 2}, {"g3_min_m", 100}, {"g3_bm", 64}, {"g3_bm", 128}, {"g3_bm", 256}, {"g3_bm", 257},
               {"g3_bm", 258}, {"g3_wide", 0}, {"g3_wide", 1}, {"g3_f8", 0}, {"no_splitk", 1}, {"no_partials", 1}, {"diag", 2}};
  // 1. single matrix: every format, row count and shape, default knobs
  for (int fmt = 0; fmt < 7; fmt++)
    for (int m : rows)
      for (const auto& s : shapes) {
        Case c;
        c.fmt = fmt, c.m = m, c.n = s[0], c.k = s[1];
        run(c);
      }
  // 2. activations x outputs (144 x 160: k no multiple of 64)
  const int shapes2[][2] = {{144, 192}, {144, 160}, {128, 1024}, {32000, 4096}};
  for (int fmt : {0, 2, 4})
    for (int m : {16, 17, 64, 65, 256, 2048})
      for (const auto& s : shapes2)
        for (int act = 0; act < 5; act++)
          for (int out = 0; out < 4; out++) {
            Case c;
            c.fmt = fmt, c.m = m, c.n = s[0], c.k = s[1], c.act = act, c.out = out;
            run(c);
          }
  // 3. every knob alone
  for (const auto& kb : knobs)
    for (int fmt : {0, 1, 2, 4})
      for (int m : {2, 33, 64, 65, 129, 2048})
        for (const auto& s : {shapes[0], shapes[1], shapes[2], shapes[4]})
          for (int out : {0, 2}) {
            Case c;
            c.fmt = fmt, c.m = m, c.n = s[0], c.k = s[1], c.out = out, c.knob = kb.name, c.kval = kb.value;
            run(c);
          }
  // 4. the fused forms
  for (const auto& kb : {knobs[0], knobs[2], knobs[3], knobs[4], knobs[11], knobs[12], knobs[14]})
    for (int fmt : {0, 1, 2, 3, 4})
      for (int m : {16, 17, 64, 65, 2048}) {
        Case b;
        b.fmt = fmt, b.m = m, b.knob = kb.name, b.kval = kb.value;
        for (int form : {2, 3})
          for (int nkv : {0, 1024})
            for (int out : {0, 1}) {
              Case c = b;
              c.form = form, c.nkv = nkv, c.out = out;
              run(c);
            }
        for (int out = 0; out < 4; out++)
          for (int act : {0, 1, 4}) {
            Case c = b;
            c.form = 7, c.n = 11008, c.out = out, c.act = act;
            run(c);
          }
        for (int neox : {0, 1})
          for (int hs : {32, 64, 128}) {
            Case c = b;
            c.form = 5, c.nkv = 1024, c.neox = neox, c.hs = hs;
            run(c);
          }
        Case c = b;
        c.form = 8, c.nkv = 1024;
        run(c);
      }
  for (int fmt : {0, 1, 3})
    for (int mis = 1; mis <= 15; mis++)
      for (int form : {2, 3, 7}) {
        Case c;
        c.fmt = fmt, c.form = form, c.mis = mis, c.n = 1024, c.k = 1024;
        run(c);
      }
  for (int brk = 1; brk <= 3; brk++) {
    Case c;
    c.form = 7, c.brk = brk, c.n = 1024, c.k = 1024;
    run(c);
  }
  for (int neox : {0, 1})
    for (int brk = 1; brk <= 31; brk++)
      for (int hs : {64, 128}) {
        Case c;
        c.form = 5, c.neox = neox, c.brk = brk, c.hs = hs, c.nkv = 1024;
        run(c);
      }
  // 5. rows whose activations cross the 2^32-byte checks: the conversion scratch (k = 4096: 524288 rows), the caller's shadow
  for (int m : {524287, 524288})
    for (int act : {0, 1})
      for (int out : {0, 2}) {
        Case c;
        c.m = m, c.n = 128, c.k = 4096, c.act = act, c.out = out;
        run(c);
      }
  return 0;
}
