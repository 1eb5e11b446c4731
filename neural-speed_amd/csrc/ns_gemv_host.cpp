// ns_gemv_host.cpp — host side of the decode kernel (gemv_kernel, ns_gemv.hip): the kernel's tuning state, and launch_gemv, which hands what
// gemv_plan (ns_gemv_plan.cpp) decided to the launcher of the weight's slice (ns_gemv.h: one translation unit of instantiations per weight
// kind and scales-per-record count); touch_gemv_module.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>

#include "../../include/ns_bestla.h"
#include "ns_common.h"
#include "ns_route.h"
#include "ns_dev.h"
#include "ns_gemv.h"

namespace ns {

#ifdef NS_TRACE
unsigned long long* trace_buffer();
#endif

static std::atomic<int> g_gemv_mode{-1};  // -1: read NS_GEMV2 once; 0 off (first-generation kernel); 1 on
void set_gemv_mode(int mode) { g_gemv_mode.store(mode); }
static int gemv_mode() {
  int m = g_gemv_mode.load();
  if (m < 0) {
    const char* e = getenv("NS_GEMV2");
    m = e ? atoi(e) : 1;
    g_gemv_mode.store(m);
  }
  return m;
}

// "gv_nw" / NS_GV_NW (diagnostics): the forced wave count of decode_waves_rule (ns_gemv_plan.cpp), which smallm_kernel shares
static std::atomic<int> g_decode_waves{0};  // ns_hip_set_tuning("gv_nw", n)
void set_decode_waves(int nw) { g_decode_waves.store(nw); }
static int forced_waves() {
  static const int env_nw0 = getenv("NS_GV_NW") ? atoi(getenv("NS_GV_NW")) : 0;
  const int forced = g_decode_waves.load();
  return forced ? forced : env_nw0;
}
int decode_waves(int grid, int ks, bool dual) { return decode_waves_rule(grid, ks, dual, forced_waves()); }

static std::atomic<int> g_gemv_rows1{-1};  // ns_hip_set_tuning("gv_rows1"): 1 (default) = launches of one row take the one-row form; -1: read NS_GV_ROWS1 once
void set_gemv_rows1(int on) { g_gemv_rows1.store(on != 0); }
bool gemv_rows1() {
  int v = g_gemv_rows1.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("NS_GV_ROWS1");
    v = e ? atoi(e) != 0 : 1;
    g_gemv_rows1.store(v);
  }
  return v != 0;
}

static std::atomic<int> g_gemv_planes{-1};  // ns_hip_set_tuning("planes"): 1 (default) = bit-plane formats stream their native records
void set_gemv_planes(int on) { g_gemv_planes.store(on != 0); }
static bool gemv_planes() {
  int v = g_gemv_planes.load();
  if (v < 0) {
    const char* e = getenv("NS_GEMV_PLANES");
    v = e ? atoi(e) != 0 : 1;
    g_gemv_planes.store(v);
  }
  return v != 0;
}

static GemvKnobs gemv_knobs() {
  static const bool i8q_off = getenv("NS_I8_INKERNEL") && atoi(getenv("NS_I8_INKERNEL")) == 0;  // A-B runs
  GemvKnobs k;
  k.gemv2 = gemv_mode();
  k.planes = gemv_planes();
  k.forced_nw = forced_waves();
  k.i8_inkernel = !i8q_off;
  return k;
}

// plan, then the launcher of the weight's slice (a slice the build leaves out is an undefined symbol when the library is linked).
// hipErrorNotSupported: outside the kernel's envelope — the caller falls back to smallm_kernel; hipErrorNotReady: it quantizes and comes back
hipError_t launch_gemv(const SmallMArgs& a, hipStream_t st) {
  GemvPlan pl = plan_gemv(a);
  return launch_gemv_planned(pl, st);
}
GemvPlan plan_gemv(const SmallMArgs& a) { return gemv_plan(a, gemv_knobs(), nullptr); }
hipError_t launch_gemv_planned(GemvPlan& pl, hipStream_t st) {
  if (pl.refusal != hipSuccess) return pl.refusal;
  GemvParams& p = pl.p;
  if (p.out_gamma) p.out_ovf = kvm_overflow_word();
#ifdef NS_TRACE
  p.trace = trace_buffer();
#endif
#define NS_SLICE(KIND, SPS) launch_gemv_##KIND##_##SPS(p, pl.scale_dt, pl.asym, pl.mode_x, pl.grid, pl.nw, pl.lds, st, pl.grid_y)
  switch (pl.kind) {
    case WK_INT4: return pl.sps == 4 ? NS_SLICE(INT4, 4) : pl.sps == 2 ? NS_SLICE(INT4, 2) : NS_SLICE(INT4, 1);
    case WK_INT8: return pl.sps == 2 ? NS_SLICE(INT8, 2) : NS_SLICE(INT8, 1);
    case WK_F8: return pl.sps == 2 ? NS_SLICE(F8, 2) : NS_SLICE(F8, 1);
    default: return pl.sps == 4 ? NS_SLICE(F4, 4) : pl.sps == 2 ? NS_SLICE(F4, 2) : NS_SLICE(F4, 1);
  }
#undef NS_SLICE
}

void touch_gemv_module() {
#define NS_GEMV_TOUCH(KIND, SPS) touch_gemv_##KIND##_##SPS();
  NS_GEMV_SLICES(NS_GEMV_TOUCH)
#undef NS_GEMV_TOUCH
}
}  // namespace ns
