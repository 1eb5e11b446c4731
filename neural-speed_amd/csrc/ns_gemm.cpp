// ns_gemm.cpp — prefill GEMM, host side: the tunables, and the launch of what gemm_plan (ns_gemm_plan.cpp) decided.  The kernels are in
// ns_gemm3.hip and ns_gemm2.hip.
#include <atomic>
#include <cstdlib>
#include <string>

#include "ns_gemm.h"

namespace ns {

// ---- tunables: ns_hip_set_tuning (ns_api.cpp) and the environment, read once per process ---------------------------------------------------
static int env_int(const char* name, int otherwise) { return getenv(name) ? atoi(getenv(name)) : otherwise; }
static std::atomic<int> g_g3_bm{0};      // "g3_bm": 0 = NS_G3_BM or automatic
static std::atomic<int> g_g3_wide{-1};   // "g3_wide" 0 / 1: -1 = NS_G3_WIDE or the default (0)
static std::atomic<int> g_g3_min_m{0};   // "g3_min_m" rows: 0 = the default (kG3MinM)
static std::atomic<int> g_g3_f8{-1};     // "g3_f8" 0 / 1: -1 = NS_G3_F8 or the default (1)
void set_gemm3_wide(int on) { g_g3_wide.store(on < 0 ? -1 : (on != 0)); }
void set_gemm3_min_m(int m) { g_g3_min_m.store(m > 0 ? m : 0); }
void set_gemm3_f8(int on) { g_g3_f8.store(on < 0 ? -1 : (on != 0)); }
// 257: 256-row tile, tall wave tiles; 258: the automatic choice without them (A-B runs)
void set_gemm3_bm(int bm) { g_g3_bm.store(bm == 64 || bm == 128 || bm == 256 || bm == 257 || bm == 258 ? bm : 0); }

static GemmKnobs gemm_knobs() {
  static const GemmKnobs env = [] {
    GemmKnobs k;
    k.v1 = getenv("NS_GEMM_V1") != nullptr;
    k.gemm3 = env_int("NS_GEMM3", 1);
    k.g3_bm = env_int("NS_G3_BM", 0);
    k.g3_wide = env_int("NS_G3_WIDE", 0);
    k.g3_f8 = env_int("NS_G3_F8", 1) != 0;
    k.no_splitk = getenv("NS_NO_SPLITK") != nullptr;
    k.diag = env_int("NS_G3_DIAG", 0);
    return k;
  }();
  GemmKnobs k = env;
  if (const int v = g_g3_min_m.load(); v > 0) k.g3_min_m = v;
  if (const int v = g_g3_bm.load(); v != 0) k.g3_bm = v;
  if (const int v = g_g3_wide.load(); v >= 0) k.g3_wide = v;
  if (const int v = g_g3_f8.load(); v >= 0) k.g3_f8 = v != 0;
  return k;
}
bool gemm3_takes(const ns_weight* w) { return gemm3_takes(w, gemm_knobs()); }

// plan, take scratch, convert, launch.  hipErrorNotSupported = another kernel serves the call (the first-generation gemm_kernel, the caller's
// general path): sizes beyond 32-bit offsets, forms the tiled kernels lack, no conversion scratch
hipError_t launch_gemm2(const SmallMArgs& a, hipStream_t st) {
  GemmKnobs kn = gemm_knobs();
  std::string why;
  GemmPlan pl = gemm_plan(a, kn, &why);
  if (pl.kernel == GK_REFUSED) return pl.refusal;
  if (pl.convert) {
    pl.p.a16 = static_cast<const _Float16*>(stream_scratch(st, pl.cvt_bytes, SLOT_A16));
    if (!pl.p.a16) return hipErrorNotSupported;
  }
  if (pl.part_bytes) {
    pl.p.part = static_cast<float*>(stream_scratch(st, pl.part_bytes, SLOT_SPLITK_PARTIALS));
    if (!pl.p.part) {  // scratch allocation failed: planned again without the K split, still correct
      const _Float16* a16 = pl.p.a16;
      kn.no_partials = true;
      pl = gemm_plan(a, kn, &why);
      pl.p.a16 = a16;
    }
  }
  if (pl.convert) {
    const hipError_t e = launch_cvt_a16(a.a, const_cast<_Float16*>(pl.p.a16), a.m, pl.p.k, a.lda, pl.kpad, st);
    if (e != hipSuccess) return e;
  }
  return pl.kernel == GK_GEMM3 ? launch_gemm3_plan(pl, st) : launch_gemm2_plan(pl, st);
}

}  // namespace ns
