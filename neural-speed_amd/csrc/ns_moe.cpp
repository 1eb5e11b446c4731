// ns_moe.cpp — host side of the mixture-of-experts family: the tuning state (moe_knobs), the expert group, the entries and their servers in
// the order ns_moe_plan.cpp gives (counters and run-time fallbacks: ns_moe_plan.h; the servers: docs/kernels/other.md, "MoE: files and paths").
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>

#include "ns_api_int.h"
#include "ns_gemv.h"
#include "ns_moe.h"
#include "ns_moe_plan.h"

namespace ns {
// the tuning keys (ns_hip_set_tuning): 0 = the environment variable if set, else the built-in value ("moe_ffn_fused": -1)
static std::atomic<int> g_gemv_rows{0}, g_grouped_rows{0}, g_ffn_grouped_rows{0}, g_ffn_fused{-1}, g_ffn_device_rows{0}, g_ffn_chunk_rows{0};
void set_moe_tuning(int what, int value) { (what == 0 ? g_gemv_rows : g_grouped_rows).store(value); }
void set_moe_ffn_fused(int on) { g_ffn_fused.store(on < 0 ? -1 : (on != 0)); }
void set_moe_ffn_grouped_rows(int rows) { g_ffn_grouped_rows.store(rows); }
void set_moe_ffn_device_rows(int rows) { g_ffn_device_rows.store(rows); }
void set_moe_ffn_chunk_rows(int rows) { g_ffn_chunk_rows.store(rows < 0 ? 0 : rows > kMoeChunkMaxRows ? kMoeChunkMaxRows : rows); }
static std::atomic<uint64_t> g_moe_stats[4], g_moe_ffn_stats[7];  // ns_hip_moe_stats, ns_hip_moe_ffn_stats / _stats_ex (ns_moe_plan.h)
static_assert(kMoeChunkALds == kGvMaxALds && kMoeChunkMaxRows == kGvMaxRows, "ns_moe_plan.h restates the decode kernel's staging limits");

static MoeKnobs moe_knobs() {
  static const MoeKnobs env = [] {
    MoeKnobs k;
    if (const char* s = getenv("NS_MOE_GEMV_ROWS")) k.gemv_rows = atoi(s);
    if (const char* s = getenv("NS_MOE_GROUPED_ROWS")) k.grouped_rows = k.ffn_grouped_rows = atoi(s);
    if (const char* s = getenv("NS_MOE_FFN_DEVICE_ROWS")) k.ffn_device_rows = atoi(s);
    return k;
  }();
  MoeKnobs k = env;
  if (const int v = g_gemv_rows.load()) k.gemv_rows = v;
  if (const int v = g_grouped_rows.load()) k.grouped_rows = v;
  if (const int v = g_ffn_grouped_rows.load()) k.ffn_grouped_rows = v;
  if (const int v = g_ffn_device_rows.load()) k.ffn_device_rows = v;
  k.ffn_fused = g_ffn_fused.load();
  k.ffn_chunk_rows = g_ffn_chunk_rows.load();
  return k;
}

bool stream_is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
  (void)hipGetLastError();
  return capturing;
}

template <class T>
static T* scratch(hipStream_t st, size_t count, int slot) { return static_cast<T*>(stream_scratch(st, count * sizeof(T), slot)); }

// ---- ns_hip_mul_mat_id's servers: 0 = done, -1 = error (set_error), 1 = not taken (nothing written to dC: the next server takes the call) ----
// Rows grouped by expert, ONE tiled GEMM per expert over its rows.  Not capturable: the id column comes back to the host once (m ints).
static int mm_grouped(const MoeParams& p, const ns_expert_group* g, int min_group_rows, hipStream_t st) {
  const int m = p.m, n = p.n, k = p.k;
  // ints: the id column [m], then src_row [pairs + 1] and pos [m] of the layout
  int32_t* ints = scratch<int32_t>(st, size_t(3) * m + 1, SLOT_MOE_IDS);
  if (!ints) return 1;
  std::vector<int32_t> col(m);
  if (!hip_ok(launch_moe_ids_column(p.ids, p.ids_stride, p.id, m, ints, st), "mul_mat_id (grouped)")) return -1;
  if (hipMemcpyAsync(col.data(), ints, size_t(m) * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return moe_fail("mul_mat_id: reading the expert ids failed");
  MoePairPlan pl;
  if (!moe_pair_plan(col.data(), 1, m, 1, p.n_as, &pl, min_group_rows)) return 1;
  const size_t rows = size_t(pl.pairs) + 1;  // (+ 1: the padding row behind a last group of one row)
  _Float16* ag = scratch<_Float16>(st, rows * k, SLOT_MOE_ROWS16);
  float* cg = scratch<float>(st, rows * n, SLOT_MOE_PRODUCTS);
  if (!ag || !cg) return 1;
  int32_t *d_src = ints + m, *d_pos = d_src + rows;
  std::vector<int32_t> tables(pl.src_row);
  tables.insert(tables.end(), pl.pos.begin(), pl.pos.end());
  if (hipMemcpyAsync(d_src, tables.data(), tables.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess)
    return moe_fail("mul_mat_id: uploading the row order failed");
  hipError_t er = launch_moe_gather(p.a, p.lda, d_src, int(rows), k, ag, st);
  for (int e = 0; e < p.n_as && er == hipSuccess; e++) {
    if (!pl.launch_rows[e]) continue;
    const size_t off = size_t(pl.offset[e]);
    SmallMArgs a{};
    a.a = nullptr, a.a16 = ag + off * k, a.lda = k, a.m = pl.launch_rows[e], a.ldc = n, a.nseg = 1, a.epilogue = NS_EPI_NONE;
    a.seg[0] = {g->experts[e], cg + off * n, nullptr};
    er = launch_gemm2(a, st);
  }
  if (er == hipSuccess) er = launch_moe_scatter(cg, d_pos, m, n, p.c, p.ldc, p.epilogue, p.d, p.ldd, st);
  const hipError_t sy = hipStreamSynchronize(st);  // the upload reads a host vector that dies with this frame
  if (er == hipErrorNotSupported) return 1;        // (nothing has been written to dC yet)
  if (!hip_ok(er, "mul_mat_id (grouped)")) return -1;
  return sy == hipSuccess ? 0 : moe_fail("mul_mat_id (grouped): launch failed");
}

// One launch of the decode kernel (ns_gemv.hip, XV = 4) per token row, the expert's base pointer picked from the table on the device.
static int mm_decode(const MoeParams& p, const ns_expert_group* g, hipStream_t st) {
  for (int t = 0; t < p.m; t++) {
    MoeRoute route{g->table, p.ids + size_t(t) * p.ids_stride + p.id, p.n_as};
    SmallMArgs a{};
    a.a = p.a + size_t(t) * p.lda, a.lda = p.lda, a.m = 1, a.ldc = p.ldc, a.nseg = 1;
    a.seg[0] = {g->experts[0], p.c + size_t(t) * p.ldc, nullptr};
    a.epilogue = p.epilogue, a.d = p.d ? p.d + size_t(t) * p.ldd : nullptr, a.ldd = p.ldd, a.moe = &route;
    const hipError_t e = launch_gemv(a, st);
    if (e == hipErrorNotSupported && t == 0) return 1;  // outside that kernel's envelope: the loop kernel serves the whole call
    if (!hip_ok(e, "mul_mat_id launch")) return -1;
  }
  return 0;
}

// ---- the block entries' servers: 0 = done, -1 = error, 1 = not taken (nothing written to out: the next server takes the call) ---------------
struct MoeFfnCall {  // the arguments of ns_hip_moe_ffn_silu / _gelu, in their order; act: NS_EPI_SILU or NS_EPI_GELU
  const float* a;
  int lda, m;
  const int32_t* ids;
  int ids_stride;
  const float* w;
  int w_stride, n_used;
  const ns_expert_group *gate, *up, *down;
  float* out;
  int ldo, act;
  hipStream_t st;
  std::string name(const char* part = "") const { return std::string(act == NS_EPI_GELU ? "moe_ffn_gelu" : "moe_ffn_silu") + part; }  // in error texts
};

// the composition: per selection three ns_hip_mul_mat_id calls (gate with the activation, up with Mul, down) and the weighted sum
static int ffn_composition(const MoeFfnCall& c) {
  const int m = c.m, ff = c.gate->experts[0]->n, dn = c.down->experts[0]->n;
  float* t1 = scratch<float>(c.st, size_t(m) * ff, SLOT_MOE_T1);
  float* t2 = scratch<float>(c.st, size_t(m) * ff, SLOT_MOE_T2);
  float* t3 = scratch<float>(c.st, size_t(m) * dn, SLOT_MOE_T3);
  if (!t1 || !t2 || !t3) return moe_fail(c.name(": scratch allocation failed"));
  for (int i = 0; i < c.n_used; i++) {
    if (ns_hip_mul_mat_id(c.a, c.ids, c.ids_stride, i, c.gate, t1, m, c.lda, ff, c.act, nullptr, 0, c.st) != 0 ||
        ns_hip_mul_mat_id(c.a, c.ids, c.ids_stride, i, c.up, t2, m, c.lda, ff, NS_EPI_MUL, t1, ff, c.st) != 0 ||
        ns_hip_mul_mat_id(t2, c.ids, c.ids_stride, i, c.down, t3, m, ff, dn, NS_EPI_NONE, nullptr, 0, c.st) != 0)
      return -1;
    const hipError_t e = launch_moe_weighted_add(c.out, c.ldo, t3, dn, c.w ? c.w + i : nullptr, c.w_stride, m, dn, i == 0, c.st);
    if (!hip_ok(e, c.name(" (weighted sum)").c_str())) return -1;
  }
  g_moe_ffn_stats[1]++;
  return 0;
}

// the fused launches: one gate / up launch over all (row, selection) pairs, then one down launch per selection
static int ffn_fused(const MoeFfnCall& c) {
  const int m = c.m, n_used = c.n_used, ff = c.gate->experts[0]->n, n_as = int(c.gate->experts.size());
  // fp32 intermediate act(gate) * up, [m][n_used][ff]: the down launches round it to fp16 while staging, like every fp32 activation row
  float* inter = scratch<float>(c.st, size_t(m) * n_used * ff, SLOT_MOE_INTER);
  if (!inter) return 1;
  MoeRoute gu_route{c.gate->table, c.ids, n_as};
  gu_route.table1 = c.up->table, gu_route.pairs = m * n_used, gu_route.nsel = n_used, gu_route.ids_stride = c.ids_stride;
  gu_route.a_stride = c.lda, gu_route.c_stride = ff;
  SmallMArgs gu{};
  gu.a = c.a, gu.lda = c.lda, gu.m = 1, gu.ldc = ff, gu.nseg = 2;
  gu.seg[0] = {c.gate->experts[0], inter, nullptr};
  gu.seg[1] = {c.up->experts[0], nullptr, nullptr};
  gu.epilogue = c.act, gu.dual = true, gu.moe = &gu_route;  // (GV_DUAL's epilogue picks SiLU or GeLU from this run-time value)
  const hipError_t e_gu = launch_gemv(gu, c.st);
  if (e_gu == hipErrorNotSupported) return 1;
  if (!hip_ok(e_gu, c.name(" (gate / up launch)").c_str())) return -1;
  for (int i = 0; i < n_used; i++) {
    MoeRoute route{c.down->table, c.ids + i, n_as};
    route.pairs = m, route.nsel = 1, route.ids_stride = c.ids_stride;
    route.w = c.w ? c.w + i : nullptr, route.w_stride = c.w_stride;
    route.a_stride = (long long)n_used * ff, route.c_stride = c.ldo, route.d_stride = c.ldo;
    SmallMArgs a{};
    a.a = inter + size_t(i) * ff, a.lda = n_used * ff, a.m = 1, a.ldc = c.ldo, a.nseg = 1;
    a.seg[0] = {c.down->experts[0], c.out, nullptr};
    a.epilogue = i ? NS_EPI_ADD : NS_EPI_NONE, a.d = i ? c.out : nullptr, a.ldd = c.ldo, a.moe = &route;
    const hipError_t e = launch_gemv(a, c.st);
    if (e == hipErrorNotSupported && i == 0) {
      g_moe_ffn_stats[2]++;  // (the gate / up launch went out; its result is dropped)
      return 1;
    }
    if (!hip_ok(e, c.name(" (down launch)").c_str())) return -1;
  }
  g_moe_ffn_stats[0]++;
  g_moe_ffn_stats[2] += uint64_t(1 + n_used);
  return 0;
}

// The grouped pass (prompt size, never captured): one read-back of the ids, moe_pair_plan, one gather into fp16 rows in group order; per
// populated expert, ascending, one gate / up pair launch of the tiled GEMM (fp16 out only) and one down launch; one combine, which alone writes out.
static int ffn_grouped(const MoeFfnCall& c) {
  const int m = c.m, n_used = c.n_used, k = c.gate->experts[0]->k, ff = c.gate->experts[0]->n, dn = c.down->experts[0]->n, n_as = int(c.gate->experts.size());
  hipStream_t st = c.st;
  // the ids, once: rows of ids_stride ints, the last one n_used long
  std::vector<int32_t> ids(size_t(m - 1) * c.ids_stride + n_used);
  if (hipMemcpyAsync(ids.data(), c.ids, ids.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    (void)hipGetLastError();
    return moe_fail(c.name(" (grouped): reading the expert ids failed"));
  }
  MoePairPlan pl;
  if (!moe_pair_plan(ids.data(), c.ids_stride, m, n_used, n_as, &pl)) return 1;
  const size_t rows = size_t(pl.pairs) + 1, n_pos = size_t(m) * n_used;  // (+ 1: the padding row behind a last group of one row)
  if (!moe_rows_addressable(rows, k, ff, dn)) return 1;
  int32_t* ints = scratch<int32_t>(st, rows + n_pos, SLOT_MOE_PAIR_INTS);
  _Float16* ag = scratch<_Float16>(st, rows * k, SLOT_MOE_PAIR_ROWS16);
  _Float16* inter = scratch<_Float16>(st, rows * ff, SLOT_MOE_PAIR_INTER16);
  float* y = scratch<float>(st, rows * dn, SLOT_MOE_PAIR_Y);
  if (!ints || !ag || !inter || !y) return 1;
  // one upload of both tables; the stream is idle (the read-back above), so waiting here costs the copy alone and the vectors may die with this frame
  std::vector<int32_t> tables(pl.src_row);
  tables.insert(tables.end(), pl.pos.begin(), pl.pos.end());
  if (hipMemcpyAsync(ints, tables.data(), tables.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    (void)hipGetLastError();
    return moe_fail(c.name(" (grouped): uploading the pair layout failed"));
  }
  hipError_t er = launch_moe_gather(c.a, c.lda, ints, int(rows), k, ag, st);
  for (int e = 0; e < n_as && er == hipSuccess; e++) {
    const int r = pl.launch_rows[e];
    if (!r) continue;
    const size_t off = size_t(pl.offset[e]);
    SmallMArgs gu{};
    gu.a = nullptr, gu.a16 = ag + off * k, gu.lda = k, gu.m = r, gu.ldc = ff, gu.nseg = 2;
    gu.seg[0] = {c.gate->experts[e], nullptr, inter + off * ff};
    gu.seg[1] = {c.up->experts[e], nullptr, nullptr};
    gu.epilogue = c.act, gu.dual = true, gu.c2 = nullptr;
    SmallMArgs dw{};
    dw.a = nullptr, dw.a16 = inter + off * ff, dw.lda = ff, dw.m = r, dw.ldc = dn, dw.nseg = 1, dw.epilogue = NS_EPI_NONE;
    dw.seg[0] = {c.down->experts[e], y + off * dn, nullptr};
    er = launch_gemm2(gu, st);
    if (er == hipSuccess) er = launch_gemm2(dw, st);
  }
  if (er == hipSuccess) er = launch_moe_combine(y, ints + rows, c.w, c.w_stride, m, n_used, dn, c.out, c.ldo, st);
  if (er == hipErrorNotSupported) return 1;
  if (!hip_ok(er, c.name(" (grouped)").c_str())) return -1;
  g_moe_ffn_stats[3]++;
  return 0;
}

// The device-grouped pass (opt-in, any stream state): nothing is read on the host.  Five launches: moe_pair_sort_kernel lays the pairs out in
// group order and cuts every group into chunks of up to R rows, for the R of each of the two K; one gather into fp16 rows; one GV_DUAL
// launch of gemv_kernel's chunk form (XV = 6) over the gate / up chunk slots, whose epilogue writes the fp16 intermediate alone; one
// GV_PLAIN launch over the down chunk slots; one combine, which alone writes out.  Both streaming launches are planned before the sort goes out.
struct MoeDevLayout {  // the ints of SLOT_MOE_DEV_INTS: [src_row P | pos P | gate / up list 1 + 3 slots_gu | down list 1 + 3 slots_dn]
  size_t pairs = 0;
  int r_gu = 0, r_dn = 0, slots_gu = 0, slots_dn = 0;
  MoeDevLayout(int m, int n_used, int n_as, int k, int gu_kstep, int ff, int dn_kstep, int cap) : pairs(size_t(m) * n_used) {
    r_gu = moe_chunk_rows(k, gu_kstep, cap), r_dn = moe_chunk_rows(ff, dn_kstep, cap);
    slots_gu = moe_chunk_slots(m, n_used, n_as, r_gu), slots_dn = moe_chunk_slots(m, n_used, n_as, r_dn);
  }
  size_t ints() const { return 2 * pairs + 2 + 3 * (size_t(slots_gu) + size_t(slots_dn)); }
  MoeDevSort sort(const int32_t* ids, int ids_stride, int n_used, int n_as, int32_t* base) const {
    int32_t* gu = base + 2 * pairs;
    return MoeDevSort{ids, ids_stride, n_used, int(pairs), n_as, r_gu, r_dn, slots_gu, slots_dn, base, base + pairs, gu, gu + 1 + 3 * size_t(slots_gu)};
  }
};

static int ffn_device_grouped(const MoeFfnCall& c, const MoeKnobs& kn) {
  const ns_weight *wg = c.gate->experts[0], *wd = c.down->experts[0];
  const int m = c.m, n_used = c.n_used, k = wg->k, ff = wg->n, dn = wd->n, n_as = int(c.gate->experts.size());
  hipStream_t st = c.st;
  const MoeDevLayout lay(m, n_used, n_as, k, wg->kstep_len, ff, wd->kstep_len, kn.ffn_chunk_rows);
  const size_t P = lay.pairs;
  int32_t* ints = scratch<int32_t>(st, lay.ints(), SLOT_MOE_DEV_INTS);
  _Float16* ag = scratch<_Float16>(st, P * k, SLOT_MOE_DEV_ROWS16);
  _Float16* inter = scratch<_Float16>(st, P * ff, SLOT_MOE_DEV_INTER16);
  float* y = scratch<float>(st, P * dn, SLOT_MOE_DEV_Y);
  if (!ints || !ag || !inter || !y) return 1;
  const MoeDevSort so = lay.sort(c.ids, c.ids_stride, n_used, n_as, ints);
  MoeRoute gu_route{c.gate->table, nullptr, n_as};
  gu_route.table1 = c.up->table, gu_route.pairs = int(P), gu_route.chunks = so.chunks_gu, gu_route.chunk_slots = lay.slots_gu;
  SmallMArgs gu{};
  gu.a16 = ag, gu.lda = k, gu.m = lay.r_gu, gu.ldc = ff, gu.nseg = 2;
  gu.seg[0] = {wg, nullptr, inter};  // (the fp16 output alone: the down launch stages fp16 rows)
  gu.seg[1] = {c.up->experts[0], nullptr, nullptr};
  gu.epilogue = c.act, gu.dual = true, gu.moe = &gu_route;
  MoeRoute dn_route{c.down->table, nullptr, n_as};
  dn_route.pairs = int(P), dn_route.chunks = so.chunks_dn, dn_route.chunk_slots = lay.slots_dn;
  SmallMArgs dw{};
  dw.a16 = inter, dw.lda = ff, dw.m = lay.r_dn, dw.ldc = dn, dw.nseg = 1, dw.epilogue = NS_EPI_NONE;
  dw.seg[0] = {wd, y, nullptr};
  dw.moe = &dn_route;
  GemvPlan plan_gu = plan_gemv(gu), plan_dn = plan_gemv(dw);
  if (plan_gu.refusal == hipErrorNotSupported || plan_dn.refusal == hipErrorNotSupported) return 1;
  if (!hip_ok(plan_gu.refusal, c.name(" (device-grouped: gate / up plan)").c_str()) || !hip_ok(plan_dn.refusal, c.name(" (device-grouped: down plan)").c_str()))
    return -1;
  hipError_t er = launch_moe_pair_sort(so, st);
  if (er == hipSuccess) er = launch_moe_gather(c.a, c.lda, so.src_row, int(P), k, ag, st);
  if (er == hipSuccess) er = launch_gemv_planned(plan_gu, st);
  if (er == hipSuccess) er = launch_gemv_planned(plan_dn, st);
  if (er == hipSuccess) er = launch_moe_combine(y, so.pos, c.w, c.w_stride, m, n_used, dn, c.out, c.ldo, st);
  if (!hip_ok(er, c.name(" (device-grouped)").c_str())) return -1;
  g_moe_ffn_stats[4]++;
  g_moe_ffn_stats[5] += 5;
  return 0;
}

// one launch can serve both weights: the same quantization format and record strides (shapes are the caller's business)
static bool one_format(const ns_weight* a, const ns_weight* b) {
  return same_quant(a, b) && a->qstride == b->qstride && a->sstride == b->sstride && a->zstride == b->zstride;
}

// the block of both activations: validation, the facts, then the servers in the plan's order
static int moe_ffn_block(const MoeFfnCall& c) {
  if (!have_device()) return -1;
  if (!c.a || !c.ids || !c.gate || !c.up || !c.down || !c.out || c.m < 1 || c.m > 65535 || c.n_used < 1 || c.n_used > c.ids_stride ||
      (c.w && c.w_stride < c.n_used))
    return moe_fail(c.name(": bad argument"));
  const ns_weight *wg = c.gate->experts[0], *wu = c.up->experts[0], *wd = c.down->experts[0];
  if (wu->n != wg->n || wu->k != wg->k || wd->k != wg->n || c.gate->experts.size() != c.up->experts.size() ||
      c.gate->experts.size() != c.down->experts.size() || c.lda < wg->k || c.ldo < wd->n)
    return moe_fail(c.name(": the gate, up and down groups do not form one feed-forward block (shapes, expert counts), or a row stride is too short"));
  const MoeKnobs kn = moe_knobs();
  MoeFacts f;
  f.gate_f8 = wg->kind == WK_F8, f.up_f8 = wu->kind == WK_F8, f.down_f8 = wd->kind == WK_F8;
  f.k = wg->k, f.ff = wg->n, f.dn = wd->n, f.n_as = int(c.gate->experts.size()), f.n_used = c.n_used, f.m = c.m;
  f.single_span = wg->single_span && wu->single_span && wd->single_span, f.gate_up_one_format = one_format(wg, wu);
  f.capturing = kn.ffn_grouped_rows > 0 && c.m >= kn.ffn_grouped_rows && stream_is_capturing(c.st);  // (asked where the plan looks at it)
  f.gu_kstep = wg->kstep_len, f.dn_kstep = wd->kstep_len, f.i8_mode = ns_hip_get_compute_mode() == NS_COMPUTE_REF_INT8;
  const MoeFfnPlan pl = moe_ffn_plan(kn, f);
  int rc = pl.fused.offered() ? ffn_fused(c) : 1;
  if (rc == 1 && pl.device.tried) {
    rc = pl.device.refused ? 1 : ffn_device_grouped(c, kn);
    if (rc == 1) g_moe_ffn_stats[6]++;
  }
  if (rc == 1 && pl.grouped.offered()) rc = ffn_grouped(c);
  return rc == 1 ? ffn_composition(c) : rc;
}

}  // namespace ns

using namespace ns;

extern "C" {

ns_expert_group* ns_hip_expert_group_create(const ns_weight* const* experts, int n_as) {
  const auto refuse = [](const char* msg) { return set_error(msg), static_cast<ns_expert_group*>(nullptr); };
  if (!experts || n_as <= 0 || n_as > 4096) return refuse("expert group: need 1..4096 experts");
  const ns_weight* w0 = experts[0];
  std::vector<MoeExpertRow> host(n_as);
  for (int i = 0; i < n_as; i++) {
    const ns_weight* w = experts[i];
    if (!w || !w0) return refuse("expert group: null weight");
    // one kernel launch serves every expert: shapes and formats must agree (they do in every MoE checkpoint)
    if (w->n != w0->n || w->k != w0->k || !one_format(w, w0) || w->shuf || w->device != w0->device)
      return refuse("expert group: experts differ in shape / format (or carry an activation shuffle)");
    host[i] = {reinterpret_cast<const uint8_t*>(w->codes), static_cast<const uint8_t*>(w->scales), w->zps};
  }
  if (w0->kind != WK_INT4 && w0->kind != WK_INT8 && w0->kind != WK_F4 && w0->kind != WK_F8)
    return refuse("expert group: S1..S8, the 4-bit float types and fp8 are supported");
  (void)moe_exp_table();  // the router's table, made outside any capture (ns_hip_moe_route); a failure is reported by that entry
  ns_expert_group* g = new ns_expert_group;
  g->experts.assign(experts, experts + n_as);
  if (hipMalloc((void**)&g->table, sizeof(MoeExpertRow) * n_as) != hipSuccess ||
      hipMemcpy(g->table, host.data(), sizeof(MoeExpertRow) * n_as, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    ns_hip_expert_group_free(g);
    return refuse("expert group: device table allocation failed");
  }
  return g;
}

void ns_hip_expert_group_free(ns_expert_group* g) {
  if (!g) return;
  if (g->table) (void)hipFree(g->table);
  delete g;
}

int ns_hip_mul_mat_id(const float* dA, const int32_t* dIds, int ids_stride, int id, const ns_expert_group* g, float* dC,
                      int m, int lda, int ldc, int epilogue, const float* dD, int ldd, void* stream) {
  if (!g || !dA || !dIds || !dC || m <= 0 || id < 0 || id >= ids_stride) return moe_fail("mul_mat_id: bad argument");
  if (m > 65535) return moe_fail("mul_mat_id: at most 65535 token rows per call");
  const ns_weight* w = g->experts[0];
  MoeParams p{};
  p.table = g->table, p.n_as = int(g->experts.size());
  p.ids = dIds, p.ids_stride = ids_stride, p.id = id;
  p.qstride = w->qstride, p.sstride = w->sstride, p.zstride = w->zstride;
  p.ksteps = w->ksteps, p.kstep_len = w->kstep_len, p.kind = w->kind;
  p.sps = w->sps, p.srows = w->srows, p.scale_dt = w->scale_dt, p.asym = w->asym ? 1 : 0;
  if (!srow_params(w, &p.srow_mul, &p.srow_shift)) return moe_fail("mul_mat_id: group size not expressible for this weight");
  p.n = w->n, p.k = w->k, p.m = m, p.a = dA, p.lda = lda, p.c = dC, p.ldc = ldc, p.epilogue = epilogue, p.d = dD, p.ldd = ldd;
  for (int i = 0; i < 16; i++) p.lut[i] = w->lutf[i];
  p.f8_e5m2 = w->qtype == DT_F8_E5M2 ? 1 : 0;
  if (size_t(w->ksteps) * w->kstep_len * 2 > 60 * 1024)  // (the loop kernel stages the whole row in LDS)
    return moe_fail("mul_mat_id: K beyond 30720 is not supported by this first version");
  hipStream_t st = (hipStream_t)stream;
  const MoeKnobs kn = moe_knobs();
  MoeFacts f;
  f.gate_f8 = w->kind == WK_F8, f.k = w->k, f.ff = w->n, f.n_as = p.n_as, f.m = m, f.single_span = w->single_span, f.shuf = w->shuf;
  if (f.gate_f8 && m > 64)  // (asked where the plan looks at it, like the capture state)
    for (const ns_weight* e : g->experts) f.all_tiled_f8 = f.all_tiled_f8 && gemm3_takes(e);
  f.capturing = kn.grouped_rows > 0 && m >= kn.grouped_rows && stream_is_capturing(st);
  const MoeMmPlan pl = moe_mm_plan(kn, f);
  if (pl.grouped.tried) {
    const int rc = pl.grouped.refused ? 1 : mm_grouped(p, g, pl.min_group_rows, st);
    if (rc == 0) g_moe_stats[0]++;
    if (rc <= 0) return rc;
    g_moe_stats[3]++;
  }
  if (pl.decode.offered()) {
    const int rc = mm_decode(p, g, st);
    if (rc == 0) g_moe_stats[1]++;
    if (rc <= 0) return rc;
  }
  if (!hip_ok(launch_moe_loop(p, w->ntiles, st), "mul_mat_id launch")) return -1;
  g_moe_stats[2]++;
  return 0;
}

void ns_hip_moe_stats(uint64_t out[4]) {
  for (int i = 0; i < 4; i++) out[i] = g_moe_stats[i].load();
}

int ns_hip_moe_ffn_silu(const float* dA, int lda, int m, const int32_t* dIds, int ids_stride, const float* dWeights, int w_stride, int n_used,
                        const ns_expert_group* gate, const ns_expert_group* up, const ns_expert_group* down, float* dOut, int ldo, void* stream) {
  return moe_ffn_block({dA, lda, m, dIds, ids_stride, dWeights, w_stride, n_used, gate, up, down, dOut, ldo, NS_EPI_SILU, (hipStream_t)stream});
}

int ns_hip_moe_ffn_gelu(const float* dA, int lda, int m, const int32_t* dIds, int ids_stride, const float* dWeights, int w_stride, int n_used,
                        const ns_expert_group* gate, const ns_expert_group* up, const ns_expert_group* down, float* dOut, int ldo, void* stream) {
  return moe_ffn_block({dA, lda, m, dIds, ids_stride, dWeights, w_stride, n_used, gate, up, down, dOut, ldo, NS_EPI_GELU, (hipStream_t)stream});
}

void ns_hip_moe_ffn_stats(uint64_t out[4]) {
  for (int i = 0; i < 4; i++) out[i] = g_moe_ffn_stats[i].load();
}

void ns_hip_moe_ffn_stats_ex(uint64_t* out, int n) {
  for (int i = 0; out && i < n; i++) out[i] = i < 7 ? g_moe_ffn_stats[i].load() : 0;
}

int ns_hip_moe_ffn_device_layout(const int32_t* dIds, int ids_stride, int m, int n_used, int n_as, int r_gu, int r_dn, int32_t* out, int n_out,
                                 void* stream) {
  if (!have_device()) return -1;
  if (!dIds || !out || m < 1 || n_used < 1 || n_used > ids_stride || n_as < 1 || int64_t(m) * n_used > kMoeDevMaxPairs || r_gu < 1 ||
      r_gu > kMoeChunkMaxRows || r_dn < 1 || r_dn > kMoeChunkMaxRows)
    return moe_fail("moe_ffn_device_layout: bad argument");
  hipStream_t st = (hipStream_t)stream;
  MoeDevLayout lay(m, n_used, n_as, 1, 1, 1, 1, 0);
  lay.r_gu = r_gu, lay.r_dn = r_dn;
  lay.slots_gu = moe_chunk_slots(m, n_used, n_as, r_gu), lay.slots_dn = moe_chunk_slots(m, n_used, n_as, r_dn);
  if (size_t(n_out) < lay.ints()) return moe_fail("moe_ffn_device_layout: the output is too short");
  int32_t* ints = scratch<int32_t>(st, lay.ints(), SLOT_MOE_DEV_INTS);
  if (!ints) return moe_fail("moe_ffn_device_layout: scratch allocation failed");
  if (!hip_ok(launch_moe_pair_sort(lay.sort(dIds, ids_stride, n_used, n_as, ints), st), "moe_ffn_device_layout")) return -1;
  if (hipMemcpyAsync(out, ints, lay.ints() * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    (void)hipGetLastError();
    return moe_fail("moe_ffn_device_layout: reading the layout failed");
  }
  return int(lay.ints());
}

}  // extern "C"
