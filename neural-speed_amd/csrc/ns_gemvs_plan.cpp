// ns_gemvs_plan.cpp — whether gemvs_kernel (ns_gemvs.hip) serves a decode call and in which decomposition: gemvs_plan, a pure function of the
// call, the tunables and the device's compute-unit count (no HIP call, no environment, no state).  ns_gemvs.cpp launches what it says;
// tests/test_stream_plan.py checks it on the CPU against the rule written out independently.
#include <algorithm>
#include <cstring>

#include "ns_gemvs.h"

namespace ns {
namespace {

// one way to cut a launch: S = 2^slices_log2 K slices of ksl k-steps x tg tile groups, ns streaming waves per workgroup
struct GvsCandidate {
  int slices_log2 = 0, ns = 0, tg = 0;
  size_t a_bytes = 0;
  bool tbl = false;
  uint32_t ksl = 0, row_stride = 0, red_wave = 0, ring_stride = 0;
  GvsLds lds{};
  double cost = 0;
};
// what every candidate of a launch shares
struct GvsShape {
  uint32_t tiles, ks;
  int rows, nq, kstep;
  bool f4;
  uint32_t slot;  // bytes of a ring slot (record_slot_bytes)
  int max_wg;     // workgroups of the launch: "gvs_grid", else one per compute unit
};

// The candidate with S slices, or false when there is none.  Its cost is in bytes a workgroup moves (the launch ends with its slowest
// workgroup): its weight records + half its activation slice (L2, about twice the HBM stream's rate per CU) + what the finalize launch of a
// split costs
bool plan_for(const GvsShape& sh, const GvsKnobs& kn, int s_log2, GvsCandidate* out) {
  const uint32_t S = 1u << s_log2, ks = sh.ks, tiles = sh.tiles;
  if (S > ks || int(S) > sh.max_wg) return false;
  GvsCandidate pl;
  pl.slices_log2 = s_log2;
  pl.ksl = (ks + S - 1) / S;
  if (uint64_t(pl.ksl) * (S - 1) >= ks) return false;  // an empty last slice
  pl.row_stride = pl.ksl * uint32_t(sh.kstep) + 8;
  pl.a_bytes = (size_t(sh.rows) * pl.row_stride * 2 + 15) & ~size_t(15);
  pl.tg = int(std::min<uint32_t>(tiles, uint32_t(sh.max_wg) / S));
  if (pl.tg < 1) return false;
  // f4: the pair table (32 KB of LDS, ~1.5 us to build and to shuffle the activations for) pays from about a hundred
  // records per workgroup on (4096 x 4096 at 8 rows, 32 records: 8.6 us with it, 8.1 without; 4096 x 14336 in 4 slices, 112
  // records: 16.4 vs 17.8; fused gate/up 14336, 256 records: 22.9 vs 27.9 — profiles/r04h_ablation.txt, r04y_table_threshold.txt)
  const uint32_t tiles_max = (tiles + uint32_t(pl.tg) - 1) / uint32_t(pl.tg);
  pl.tbl = sh.f4 && kn.gvs_table != 0 && (kn.gvs_table > 0 || uint64_t(tiles_max) * pl.ksl * sh.nq >= 96u);
  pl.red_wave = uint32_t(sh.nq) * uint32_t((sh.rows + 3) / 4) * 256u;
  // streaming waves: as many as LDS holds and the workgroup has units for (units are dealt round-robin: any count
  // balances); the time of a workgroup ~ its units / waves, padded when there are fewer units than waves
  auto ring_of = [&](int ns) {
    const size_t items = (size_t(pl.ksl) * tiles_max + ns - 1) / ns * sh.nq;
    return (std::min<size_t>(items, size_t(kGsPF)) * sh.slot + 15) & ~size_t(15);
  };
  for (int ns = kGsMaxNS; ns >= 1 && pl.ns == 0; ns--) {
    if (kn.gvs_waves > 0 && ns != std::min(kn.gvs_waves, kGsMaxNS)) continue;
    if (kn.gvs_waves <= 0 && uint32_t(ns) > std::max<uint32_t>(1u, pl.ksl * tiles_max)) continue;
    const GvsLds l = gvs_lds(pl.tbl, pl.a_bytes, size_t(ns) * pl.red_wave, ns, ring_of(ns));
    if (l.bytes > kGsMaxLds) continue;
    pl.ns = ns;
    pl.ring_stride = uint32_t(ring_of(ns));
    pl.lds = l;
  }
  if (pl.ns == 0) return false;
  const double t = double(pl.ksl) * (1.0 + 0.5 * std::max(0, 12 - pl.ns) / 12.0);
  // + a fixed cost per tile of a workgroup (flush, reduction, epilogue or slab store: about 8 KB of streaming each: the service wave needs ~0.8 us per tile)
  pl.cost = double(tiles_max) * (t * sh.nq * sh.slot + 8e3) + 0.5 * double(pl.a_bytes) + (S > 1 ? 75e3 : 0.0);
  *out = pl;
  return true;
}

// the cheapest candidate over S = 1 .. 32 ("gvs_slices": that S alone); ties go to the fewer slices
bool best_candidate(const GvsShape& sh, const GvsKnobs& kn, GvsCandidate* best) {
  bool have = false;
  for (int s_log2 = 0; s_log2 <= 5; s_log2++) {
    if (kn.gvs_slices > 0 && (1 << s_log2) != kn.gvs_slices) continue;
    GvsCandidate pl;
    if (!plan_for(sh, kn, s_log2, &pl)) continue;
    if (!have || pl.cost < best->cost) *best = pl, have = true;
  }
  return have;
}

// which kernel by shape (profiles/r04n_rows.txt, us, one-tile-per-workgroup gemv_kernel -> this kernel).  This kernel's time
// hardly depends on the row count, gemv_kernel's grows with the activations every tile stages; gemv_kernel's prologue is
// about 0.7 us leaner, so short launches of a few rows stay there:
//   4096 x 4096 int4      2 rows 5.6 -> 6.2    6 rows 6.1 -> 6.8    12 rows 8.5 -> 7.4   16 rows 9.0 -> 7.4
//   gate/up 11008 int4    2 rows 13.5 -> 15.2  4 rows 15.3 -> 16.2  6 rows 19.0 -> 16.7  12 rows 20.2 -> 17.6
//   gate/up 14336 nf4     2 rows 22.7 -> 20.8  6 rows 27.4 -> 21.4  16 rows 39.2 -> 28.7
//   4096 x 11008 int4     2 rows 8.7 -> 9.0    3 rows 11.5 -> 9.3 (66 KB of activations: beyond gemv_kernel)   16 rows 24.8 -> 14.3
bool shape_rule(const GvsShape& sh, bool dual) {
  const bool beyond_gemv = size_t(sh.rows) * (size_t(sh.ks) * sh.kstep + 8) * 2 > 64 * 1024;  // gemv_kernel's activation envelope
  const bool wide = dual || sh.tiles >= 512;
  return beyond_gemv || (sh.f4 && wide) || (sh.rows >= 5 && wide) || sh.rows >= 9;
}

// nullptr, or what keeps the call from this kernel.  fp16 activations with 16-byte aligned rows; several rows need K to fill whole k-steps
// (a row's padding columns would otherwise read the next row through the descriptor).  A caller without the fp16 shadow (the reference's
// device graph hands over fp32 tensors) gets one conversion pass into scratch first (round to nearest even, what the shadow's producers
// do: bit-identical results either way, tests/test_gpu_fullsize.py)
const char* outside_envelope(const SmallMArgs& a, const GvsKnobs& kn, StreamTable* t) {
  if (kn.gvs == 0 || a.m < (kn.gvs == 2 ? 1 : 2) || a.m > kGsMaxRows) return "gvs 0, or rows outside the kernel's range";
  if (a.link || a.rope || a.i8 || a.moe) return "carried norm, fused RoPE, int8-reference numerics and expert launches are gemv_kernel's";
  if (a.nseg < 1 || a.nseg > 3 || (a.dual && a.nseg != 2)) return "one to three matrices; gate/up pairs are two";
  const ns_weight* w0 = a.seg[0].w;
  const bool shadow = a.a16 != nullptr;
  if (shadow ? ((a.lda & 7) || (reinterpret_cast<uintptr_t>(a.a16) & 15)) : (a.a == nullptr)) return "activations: an fp16 shadow with 16-byte rows, or fp32 rows to convert";
  if ((w0->k & 7) || (a.m > 1 && w0->k % w0->kstep_len != 0)) return "K: a multiple of 8, and of the k-step for several rows";
  if (uint64_t(a.m) * uint64_t(shadow ? a.lda : w0->k) * 2 >= (uint64_t(1) << 30)) return "activations beyond 30-bit staging offsets";
  if (!stream_table(a, [](const ns_weight* w) { return w; }, t)) return "a matrix is not one allocation below 2 GiB";
  for (int i = 0; i < a.nseg; i++) {
    if (!same_stream_layout(a.seg[i].w, w0)) return "the matrices differ in format or layout";
    if (a.dual && a.seg[i].w->ntiles != w0->ntiles) return "gate/up pairs of different widths";
  }
  if (t->tiles == 0 || w0->ksteps == 0) return "an empty launch";
  return nullptr;
}

// everything of GvsParams and GvsFinParams but the launcher's pointers
void fill_params(const SmallMArgs& a, const StreamTable& t, const GvsCandidate& c, int mul, int shift, GvsPlan* pl) {
  const ns_weight* w0 = a.seg[0].w;
  const bool mseg = pl->mode == GS_MSEG;
  GvsParams& p = pl->p;
  for (int i = 0; i < a.nseg; i++) p.mat[i] = t.mat[i];
  p.wb0 = t.wb[0], p.wb1 = t.wb[1], p.wb2 = t.wb[2];
  p.a = pl->convert ? nullptr : a.a16;
  p.so0 = t.soff[0], p.so1 = t.soff[1], p.so2 = t.soff[2];
  p.zo0 = t.zoff[0], p.zo1 = t.zoff[1], p.zo2 = t.zoff[2];
  p.ks = uint32_t(w0->ksteps), p.ksl = c.ksl, p.s_log2 = uint32_t(c.slices_log2);
  p.qstride = w0->qstride, p.sstride = w0->sstride, p.zstride = w0->zstride;
  p.srows = uint32_t(w0->srows), p.srow_mul = uint32_t(mul), p.srow_shift = uint32_t(shift);
  p.tb1 = mseg ? t.tbeg[1] : 0xffffffffu;
  p.tb2 = (mseg && a.nseg > 2) ? t.tbeg[2] : 0xffffffffu;
  p.ntiles = t.tiles;
  p.tg_count = uint32_t(c.tg), p.tiles_base = t.tiles / uint32_t(c.tg), p.tiles_rem = t.tiles % uint32_t(c.tg);
  p.ns = uint32_t(c.ns);
  p.m = a.m, p.k = w0->k, p.lda = pl->convert ? w0->k : a.lda;
  p.row_stride = c.row_stride;
  p.a_off = uint32_t(c.lds.a_off), p.a_bytes = uint32_t(c.a_bytes);
  p.ctl_off = uint32_t(c.lds.ctl_off), p.red_off = uint32_t(c.lds.red_off), p.ring_off = uint32_t(c.lds.ring_off);
  p.ring_stride = c.ring_stride;
  p.red_wave = c.red_wave, p.red_slot = uint32_t(c.ns) * c.red_wave;
  p.c2 = a.c2, p.d = a.d, p.ldc = a.ldc, p.ldd = a.ldd, p.epilogue = a.epilogue;
  const uint32_t nq = a.dual ? 2 : 1;
  p.slab_bytes = uint32_t((size_t(1) << c.slices_log2) * t.tiles * nq * 256 * sizeof(float));
  if (w0->kind == WK_F4) {
    f4_lut_planes(w0->lut, &p.lut);
    for (int i = 0; i < 8; i++)
      p.lut16[i] = uint32_t(__builtin_bit_cast(unsigned short, w0->lut[2 * i])) | (uint32_t(__builtin_bit_cast(unsigned short, w0->lut[2 * i + 1])) << 16);
  }
  p.f8 = f8_consts(w0->qtype);
  GvsFinParams& f = pl->f;
  f.slices = 1u << c.slices_log2, f.ntiles = t.tiles, f.nq = nq;
  f.tb1 = p.tb1, f.tb2 = p.tb2;
  f.m = a.m;
  for (int i = 0; i < 3; i++) f.mat[i] = p.mat[i];
  f.c2 = a.c2, f.d = a.d, f.ldc = a.ldc, f.ldd = a.ldd, f.epilogue = a.epilogue;
}

}  // namespace

GvsPlan gemvs_plan(const SmallMArgs& a, const GvsKnobs& kn, int cus, std::string* why) {
  GvsPlan pl;
  memset(&pl.p, 0, sizeof(pl.p));
  memset(&pl.f, 0, sizeof(pl.f));
  auto refuse = [&](const char* reason) {
    if (why) *why = reason;
    return pl;
  };
  StreamTable t;
  if (const char* miss = outside_envelope(a, kn, &t)) return refuse(miss);
  const ns_weight* w0 = a.seg[0].w;
  int mul, shift;
  if (!srow_params(w0, &mul, &shift)) return refuse("the scale-row rule is not a multiply and a shift");
  const GvsShape sh{t.tiles, uint32_t(w0->ksteps), a.m, a.dual ? 2 : 1, w0->kstep_len, w0->kind == WK_F4, record_slot_bytes(w0),
                    kn.gvs_grid > 0 ? kn.gvs_grid : cus};
  if (kn.gvs == 1 && !shape_rule(sh, a.dual)) return refuse("by shape: gemv_kernel serves this call");
  GvsCandidate best;
  if (!best_candidate(sh, kn, &best)) return refuse("no decomposition fits the workgroups and LDS");
  const uint32_t S = 1u << best.slices_log2;
  const size_t slab_bytes = size_t(S) * t.tiles * sh.nq * 256 * sizeof(float);
  if (S > 1 && slab_bytes >= (size_t(1) << 31)) return refuse("split-K partial sums beyond 2 GiB");

  pl.kind = w0->kind, pl.sps = w0->sps, pl.scale_dt = w0->scale_dt, pl.asym = w0->asym;
  pl.mode = a.dual ? GS_DUAL : (a.nseg > 1 ? GS_MSEG : GS_PLAIN);
  pl.convert = a.a16 == nullptr;
  pl.cvt_bytes = pl.convert ? size_t(a.m) * w0->k * 2 : 0;
  pl.slab_bytes = S > 1 ? slab_bytes : 0;
  // Who adds the slices: a second launch (gemvs_finalize_kernel, the default) or — "gvs_finalize" 0 — the tile's owner inside
  // the launch, behind one self-resetting ticket per tile unit.  Measured equal (profiles/r04u_split_k_finish.txt: 4096 x 14336
  // at 8 rows 17.1 vs 17.3 us with 2 slices, 17.8 vs 17.8 with 4): what the in-launch finish saves in launch boundary the owner
  // spends reading the other slices past the caches; it also needs every workgroup of the launch resident at once (an owner
  // spins on tickets other workgroups draw), which a second launch does not — hence the default.
  pl.want_tickets = S > 1 && !kn.gvs_finalize && t.tiles <= kGsTicketCap;
  pl.want_table_image = best.tbl && kn.table_dma;
  fill_params(a, t, best, mul, shift, &pl);
  pl.grid = best.tg * int(S);
  pl.nwaves = best.ns + 1;
  pl.lds = best.lds.bytes;
  pl.cost = best.cost;
  pl.refusal = hipSuccess;
  return pl;
}

}  // namespace ns
