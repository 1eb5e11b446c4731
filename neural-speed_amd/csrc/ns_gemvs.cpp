// ns_gemvs.cpp — gemvs_kernel, host side: the tunables, the device's compute-unit count, the f4 pair-table images, and the launch of what
// gemvs_plan (ns_gemvs_plan.cpp) decided.  The kernels are in ns_gemvs.hip.
#include <array>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

#include "ns_gemvs.h"

namespace ns {

#ifdef NS_TRACE
unsigned long long* trace_buffer();
#endif

// ---- tunables (ns_hip_set_tuning): "gvs" 0 = off, 1 = by shape (default), 2 = always from 1 row, 3 = always from 2 rows; "gvs_slices" /
//      "gvs_waves" / "gvs_grid" force the decomposition (0 = by shape); "gvs_table"; "gvs_finalize".  A stored value below a knob's range makes
//      the next read consult the environment again ----
struct GvsKnob {
  std::atomic<int> value;
  const char* env;
  int dflt;
};
static GvsKnob g_knobs[6] = {{{-1}, "NS_GVS", 1},        {{-1}, "NS_GVS_SLICES", 0}, {{-1}, "NS_GVS_WAVES", 0},
                             {{-1}, "NS_GVS_GRID", 0},   {{-2}, "NS_GVS_TABLE", -1}, {{-1}, "NS_GVS_FINALIZE", 1}};
void set_gemvs_tuning(int what, int value) { g_knobs[what >= 0 && what < 5 ? what : 5].value.store(value); }
static int gvs_knob(int what) {
  GvsKnob& k = g_knobs[what];
  int v = k.value.load();
  if (v < (k.dflt < 0 ? -1 : 0)) {
    const char* e = getenv(k.env);
    v = e ? atoi(e) : k.dflt;
    k.value.store(v);
  }
  return v;
}
static GvsKnobs gvs_knobs() {
  static const bool dma_off = getenv("NS_GVS_TABLE_DMA") && atoi(getenv("NS_GVS_TABLE_DMA")) == 0;  // A-B runs
  GvsKnobs k;
  k.gvs = gvs_knob(0), k.gvs_slices = gvs_knob(1), k.gvs_waves = gvs_knob(2), k.gvs_grid = gvs_knob(3);
  k.gvs_table = gvs_knob(4), k.gvs_finalize = gvs_knob(5);
  k.table_dma = !dma_off;
  return k;
}
static int gvs_cus() {
  static const int cus = [] {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    return prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }();
  return cus;
}

// ---- f4 pair-table images: entry e = {value[e & 15], value[e >> 4]} as two fp16, 32 bank copies each — what the kernel's build_table
//      writes.  One image per value table (NF4 / FP4-BNB / FP4-E2M1), created on the first launch that wants it OUTSIDE a stream
//      capture (an allocation + a synchronous copy); a launch that finds none gets nullptr and builds the table with its waves ----
static std::mutex g_tbl_mu;
static std::map<std::array<uint16_t, 16>, void*> g_tbl_img;
static const void* gvs_f4_table_image(const uint32_t* lut16, hipStream_t st) {
  std::array<uint16_t, 16> key;
  for (int i = 0; i < 16; i++) key[i] = uint16_t(lut16[i / 2] >> (16 * (i & 1)));
  std::lock_guard<std::mutex> lk(g_tbl_mu);
  auto it = g_tbl_img.find(key);
  if (it != g_tbl_img.end()) return it->second;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return nullptr;
  }
  std::vector<uint32_t> img(kGsTblBytes / 4);
  for (uint32_t e = 0; e < 256; e++)
    for (uint32_t c = 0; c < 32; c++) img[e * 32 + c] = uint32_t(key[e & 15]) | (uint32_t(key[e >> 4]) << 16);
  void* d = nullptr;
  if (hipMalloc(&d, kGsTblBytes) != hipSuccess || hipMemcpy(d, img.data(), kGsTblBytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    if (d) (void)hipFree(d);
    return nullptr;  // (not cached: tried again next time)
  }
  g_tbl_img.emplace(key, d);
  return d;
}

// plan, take scratch, convert, launch, finalize.  hipErrorNotSupported: outside the kernel's envelope, not the better decomposition, or no
// scratch — the caller goes on to gemv_kernel
hipError_t launch_gemvs(const SmallMArgs& a, hipStream_t st) {
  GvsPlan pl = gemvs_plan(a, gvs_knobs(), gvs_cus(), nullptr);
  if (pl.refusal != hipSuccess) return pl.refusal;
  GvsParams& p = pl.p;
  if (pl.slab_bytes) {
    p.slab = static_cast<float*>(stream_scratch(st, pl.slab_bytes, SLOT_SPLITK_PARTIALS));
    if (!p.slab) return hipErrorNotSupported;
    if (pl.want_tickets) p.tickets = static_cast<uint32_t*>(stream_scratch_zeroed(st, size_t(kGsTicketCap) * 4, SLOT_GEMVS_TICKETS));
  }
  if (pl.convert) {
    void* sc = stream_scratch(st, pl.cvt_bytes, SLOT_A16);
    if (!sc) return hipErrorNotSupported;
    const hipError_t ce = launch_cvt_a16(a.a, sc, a.m, p.k, a.lda, p.k, st);
    if (ce != hipSuccess) return ce;
    p.a = sc;
  }
  if (pl.want_table_image) p.tbl_img = gvs_f4_table_image(p.lut16, st);
#ifdef NS_TRACE
  p.trace = trace_buffer();
#endif
  static const bool dbg = getenv("NS_GVS_DEBUG") != nullptr;
  if (dbg)
    fprintf(stderr, "gemvs: m %d tiles %u ks %u mode %d -> slices %u (ksl %u) groups %d waves %d lds %zu (A %zu) cost %.0f\n", a.m, p.ntiles, p.ks,
            pl.mode, 1u << p.s_log2, p.ksl, int(p.tg_count), int(p.ns), pl.lds, size_t(p.a_bytes), pl.cost);
  if (dbg && pl.kind == WK_F4) fprintf(stderr, "gemvs: f4 pair table %s\n", p.a_off ? "on" : "off");

  const hipError_t e = launch_gemvs_plan(pl, st);
  if (e != hipSuccess || !pl.slab_bytes || p.tickets) return e;
  pl.f.slab = p.slab;
  return launch_gemvs_finalize(pl, st);
}

}  // namespace ns
