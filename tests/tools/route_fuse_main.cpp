// Program of tests/test_route_fuse.py: runs the device route's planner (neural-speed_amd/csrc/ns_route_fuse.cpp, compiled into this program alone) on
// op traces of a llama layer stack built from made-up addresses and prints what it decided, one block per case:
//   case <name>
//   k <kind of every op of the trace>
//   diff ok <act_delta> <number of activation pointers>   |   diff no <op> <why>
//   p <op> <moving> <delta> <pshift>                        (cases that are about the token diff)
//   x <kind> <idx,..> <in_link> <out_link> <a16> <o16> <slot of a16p> <slot of o16p> <aux>
//   links <carried norms> <shadows> <bytes> <rope table offset>
//   seg <beg> <end> <xbeg> <xend>
// Host code only: no HIP call is made, no tensor exists.  The RouteEnv is a table: which caches have a mirror, which weights may carry a norm, a
// scratch that can be told to fail.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ns_route_fuse.cpp"

using namespace ns;

namespace {

constexpr long long HS = 128, HEADS = 2, D = 256, FF = 512, NCTX = 64;
constexpr uintptr_t kPool = 0x10000000, kWeights = 0x40000000, kCache = 0x50000000, kScratch = 0x70000000;
constexpr long long kTokenShift = 0x20000;  // the reference's pool: a token's activations sit this far above the previous token's
// a layer is 20 ops: norm mul | K rope cpy V cpy Q rope | attn | wo add | norm mul | w1 silu w3 mul | w2 add; behind the last one norm mul and the output projection

struct Cfg {
  int layers = 2;
  long long m = 1, n_past = 5, heads_kv = 2, n_dims = HS;
  bool yarn = false, k_f16 = false;
  int order = 0;              // address order of the q / k / v rows: 0 q k v, 1 k q v
  long long v_gap = 0;        // bytes between the k rows' end and v (unequal spacing)
  long long spacing = 0;      // != 0: q, k, v this many bytes apart whatever their width
  int extra = 0;              // one more op at the token's end: 1 reads layer 0's raw wo result, 2 layer 0's raw w1 result, 3 rewrites the wo result, then reads it
  int mha_seq = 0;            // != 0: the attention's seq
  bool foreign_write = false;  // the last add stores into layer 0's K cache
};
struct Env : RouteEnv {
  bool mirrors = true;
  int refuse = -1;  // index into Model::w of a weight that may not carry a norm
  const ns_weight* refused = nullptr;
  int fail_slot = -1;
  int layers = 0;
  long long heads_kv = 2;
  static long long cache_bytes() { return HEADS * NCTX * HS * 4; }
  bool mirror_of_cell(const void* cell, KvMirrorArgs* out) override {
    const uintptr_t c = reinterpret_cast<uintptr_t>(cell);
    if (!mirrors || c < kCache || c >= kCache + uintptr_t(2 * layers * cache_bytes())) return false;
    const long long which = (c - kCache) / cache_bytes();  // K of layer 0, V of layer 0, K of layer 1, ...
    *out = KvMirrorArgs{};
    out->base32 = reinterpret_cast<const char*>(kCache + which * cache_bytes());
    out->m16 = reinterpret_cast<_Float16*>(kScratch + 0x1000000 + which * cache_bytes());
    out->elems = heads_kv * NCTX * HS, out->n_ctx = NCTX, out->hs = HS, out->transposed = int(which & 1);
    return true;
  }
  bool mirror_for_producer(const void*, const void*, int, int, int, int, int, _Float16** k16, _Float16** v16) override {
    *k16 = *v16 = reinterpret_cast<_Float16*>(kScratch + 0x1000000);
    return mirrors;
  }
  void* scratch(size_t, int slot) override { return slot == fail_slot ? nullptr : reinterpret_cast<void*>(kScratch + 0x1000 * slot); }
  bool weight_carries_norm(const ns_weight* w) override { return w != refused; }
};
int slot_of(const void* p) { return p ? int((reinterpret_cast<uintptr_t>(p) - kScratch) / 0x1000) : 0; }

struct Model {
  std::vector<ns_weight> w;  // per layer: wk wv wq wo w1 w3 w2; then the output projection
  explicit Model(const Cfg& c) : w(size_t(7 * c.layers + 1)) {
    for (int l = 0; l < c.layers; l++) {
      const long long nk[7][2] = {{c.heads_kv * HS, D}, {c.heads_kv * HS, D}, {D, D}, {D, D}, {FF, D}, {FF, D}, {D, FF}};
      for (int t = 0; t < 7; t++) w[7 * l + t].n = int(nk[t][0]), w[7 * l + t].k = int(nk[t][1]);
    }
    w.back().n = 1024, w.back().k = int(D);
  }
};

// one token's trace, the way the reference's graph hands a llama layer stack over
std::vector<RouteOp> token(const Cfg& c, const Model& md, int t) {
  std::vector<RouteOp> ops;
  const long long M = c.m, np = c.n_past + t, hkv = c.heads_kv;
  uintptr_t next = kPool + uintptr_t(t * kTokenShift);
  auto alloc = [&](long long floats) {
    const uintptr_t p = next;
    next += uintptr_t((floats * 4 + 255) / 256 * 256);
    return reinterpret_cast<float*>(p);
  };
  auto at = [](const float* base, long long bytes) { return reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(base) + uintptr_t(bytes)); };
  auto mat = [&](long long n, long long ne[4], long long nb[4]) { ne[0] = n, ne[1] = M, ne[2] = ne[3] = 1, nb[0] = 4, nb[1] = 4 * n, nb[2] = nb[3] = 4 * n * M; };
  auto vec = [&](long long n, long long ne[4], long long nb[4]) { ne[0] = n, ne[1] = ne[2] = ne[3] = 1, nb[0] = 4, nb[1] = nb[2] = nb[3] = 4 * n; };
  long long ne[4], nb[4], ve[4], vb[4], fe[4], fb[4];
  mat(D, ne, nb), vec(D, ve, vb), mat(FF, fe, fb);
  const float* gamma = reinterpret_cast<const float*>(kWeights + 0x100000);
  auto rope = [&](float* x, long long heads) {
    return c.yarn ? route_op_rope_yarn(x, x, 1, M, heads, HS, np, c.n_dims, 0, 10000.f, 1.f, 4096, 1.f, 1.f, 32.f, 1.f)
                  : route_op_rope(x, x, 1, M, heads, HS, np, c.n_dims, 0, 10000.f, 1.f, 0.f, 1.f);
  };
  float* x = alloc(M * D);
  float *raw_wo0 = nullptr, *raw_w10 = nullptr;
  for (int l = 0; l < c.layers; l++) {
    const ns_weight* w = &md.w[size_t(7 * l)];
    float* kc = reinterpret_cast<float*>(kCache + uintptr_t((2 * l) * Env::cache_bytes()));
    float* vc = reinterpret_cast<float*>(kCache + uintptr_t((2 * l + 1) * Env::cache_bytes()));
    float *pn = alloc(M * D), *ph = alloc(M * D);
    // the q / k / v rows: one block, in the configured address order
    const long long qb = M * HEADS * HS * 4, kb = M * hkv * HS * 4, step = c.spacing ? c.spacing : qb;
    float* blk = alloc(3 * M * D + c.v_gap / 4);
    float *pq, *pk, *pv;
    if (c.order == 0) pq = blk, pk = at(blk, c.spacing ? step : qb), pv = at(pk, step + c.v_gap);
    else pk = blk, pq = at(blk, c.spacing ? step : kb), pv = at(pq, (c.spacing ? step : kb) + c.v_gap);
    ops.push_back(route_op_rms_norm(x, pn, M, D, 1e-5f));
    ops.push_back(route_op_binary(RK_MUL, pn, gamma, ph, ne, nb, ve, vb, nb));
    ops.push_back(route_op_gemm(ph, &w[0], pk, M, hkv * HS, D, D, D));
    ops.push_back(rope(pk, hkv));
    {  // K -> cache [head][n_ctx][hs] from position np on
      const long long e[4] = {HS, M, hkv, 1}, s[4] = {4, hkv * HS * 4, HS * 4, hkv * HS * 4 * M}, d[4] = {4, HS * 4, NCTX * HS * 4, hkv * NCTX * HS * 4};
      ops.push_back(route_op_dup(pk, at(kc, np * HS * 4), e, s, d, c.k_f16));
    }
    ops.push_back(route_op_gemm(ph, &w[1], pv, M, hkv * HS, D, D, D));
    {  // V -> cache [head][hs][n_ctx]
      const long long e[4] = {M, HS, hkv, 1}, s[4] = {hkv * HS * 4, 4, HS * 4, hkv * HS * 4 * M}, d[4] = {4, NCTX * 4, HS * NCTX * 4, hkv * HS * NCTX * 4};
      ops.push_back(route_op_dup(pv, at(vc, np * 4), e, s, d, false));
    }
    ops.push_back(route_op_gemm(ph, &w[2], pq, M, D, D, D, D));
    ops.push_back(rope(pq, HEADS));
    float* pa = alloc(M * D);
    const long long seq = c.mha_seq ? c.mha_seq : M;
    ops.push_back(route_op_mha(pq, kc, vc, pa, 1, seq, np + seq, HEADS, hkv, HS, NCTX, 0.0884f, 1));
    float *pt = alloc(M * D), *pr = alloc(M * D);
    ops.push_back(route_op_gemm(pa, &w[3], pt, M, D, D, D, D));
    ops.push_back(route_op_binary(RK_ADD, pt, x, pr, ne, nb, ne, nb, nb));
    float *pn2 = alloc(M * D), *ph2 = alloc(M * D);
    ops.push_back(route_op_rms_norm(pr, pn2, M, D, 1e-5f));
    ops.push_back(route_op_binary(RK_MUL, pn2, gamma, ph2, ne, nb, ve, vb, nb));
    float *pt1 = alloc(M * FF), *ps = alloc(M * FF), *pt3 = alloc(M * FF), *pp = alloc(M * FF);
    ops.push_back(route_op_gemm(ph2, &w[4], pt1, M, FF, D, D, FF));
    ops.push_back(route_op_silu(pt1, ps, M * FF));
    ops.push_back(route_op_gemm(ph2, &w[5], pt3, M, FF, D, D, FF));
    ops.push_back(route_op_binary(RK_MUL, ps, pt3, pp, fe, fb, fe, fb, fb));
    float *pt2 = alloc(M * D), *po = alloc(M * D);
    ops.push_back(route_op_gemm(pp, &w[6], pt2, M, D, FF, FF, D));
    ops.push_back(route_op_binary(RK_ADD, pt2, pr, c.foreign_write && l == c.layers - 1 ? reinterpret_cast<float*>(kCache) : po, ne, nb, ne, nb, nb));
    x = po;
    if (l == 0) raw_wo0 = pt, raw_w10 = pt1;
  }
  float *pn = alloc(M * D), *ph = alloc(M * D), *logits = alloc(M * 1024);
  ops.push_back(route_op_rms_norm(x, pn, M, D, 1e-5f));
  ops.push_back(route_op_binary(RK_MUL, pn, gamma, ph, ne, nb, ve, vb, nb));
  ops.push_back(route_op_gemm(ph, &md.w.back(), logits, M, 1024, D, D, 1024));
  float* spare = alloc(M * FF);
  if (c.extra == 3) ops.push_back(route_op_silu(logits, raw_wo0, M * D));
  if (c.extra == 1 || c.extra == 3) ops.push_back(route_op_binary(RK_ADD, raw_wo0, logits, spare, ne, nb, ne, nb, nb));
  if (c.extra == 2) ops.push_back(route_op_silu(raw_w10, spare, M * FF));
  return ops;
}

std::vector<PlanOp> as_plan(const std::vector<RouteOp>& ops) {
  std::vector<PlanOp> w(ops.size());
  for (size_t j = 0; j < w.size(); j++) w[j] = PlanOp{ops[j], 0, 0, 0u};
  return w;
}
void print_kinds(const std::vector<RouteOp>& ops) {
  printf("k");
  for (const RouteOp& o : ops) printf(" %u", o.kind);
  printf("\n");
}
void print_launches(const std::vector<ExecOp>& x) {
  static const char* names[] = {"OP", "QKV", "ROPE2", "DUP2", "GEMM_ADD", "GATEUP", "ROPE_APPEND", "QKV_ROPE", "ROPE_TABLE", "NORM16", "QKV_ROPE_M"};
  for (const ExecOp& e : x) {
    printf("x %s ", names[e.xk]);
    for (int q = 0; q < kXIdx; q++) printf("%s%d", q ? "," : "", e.idx[q]);
    printf(" %d %d %d %d %d %d %d\n", e.in_link, e.out_link, e.a16, e.o16, slot_of(e.a16p), slot_of(e.o16p), e.aux);
  }
}
void print_segments(const std::vector<SegmentCut>& segs) {
  for (const SegmentCut& s : segs) printf("seg %d %d %d %d\n", s.beg, s.end, s.xbeg, s.xend);
}

// a plan from two consecutive tokens of one configuration
void plan_case(const char* name, const Cfg& c, void (*tune)(RouteKnobs&, Env&) = nullptr, bool print_plan = false, int seg = 0, int seg0 = 0) {
  const Model md(c);
  Env env;
  env.layers = c.layers, env.heads_kv = c.heads_kv;
  RouteKnobs kn;
  if (tune) tune(kn, env);
  if (env.refuse >= 0) env.refused = &md.w[size_t(env.refuse)];
  const std::vector<RouteOp> t0 = token(c, md, 0), t1 = token(c, md, 1);
  printf("case %s\n", name);
  print_kinds(t1);
  TokenPlan tp;
  const NoPlan no = diff_tokens(t0, t1, env, &tp);
  if (no.why) {
    printf("diff no %ld %s\n", no.at, no.why);
    return;
  }
  printf("diff ok %lld %zu\n", tp.act_delta, tp.act_ptrs.size());
  if (print_plan)
    for (size_t j = 0; j < tp.ops.size(); j++) printf("p %zu %d %lld %u\n", j, tp.ops[j].moving, tp.ops[j].delta, tp.ops[j].pshift);
  LinkPlan lp;
  const std::vector<ExecOp> x = plan_launches(tp.ops, kn, env, links_wanted(kn), &lp);
  print_launches(x);
  printf("links %zu %zu %zu %zu\n", lp.links.size(), lp.shadows.size(), lp.bytes, lp.rope_tab_off);
  if (seg) {
    kn.seg = seg, kn.seg0 = seg0;
    print_segments(cut_segments(x, tp.ops, kn));
  }
}
// the two traces handed to the diff differ in more than a token's step
void diff_case(const char* name, const Cfg& c0, const Cfg& c1, void (*edit)(std::vector<RouteOp>&) = nullptr) {
  const Model md(c0);
  Env env;
  env.layers = c0.layers, env.heads_kv = c0.heads_kv;
  std::vector<RouteOp> t0 = token(c0, md, 0), t1 = token(c1, md, 1);
  if (edit) edit(t1);
  printf("case %s\n", name);
  print_kinds(t1);
  TokenPlan tp;
  const NoPlan no = diff_tokens(t0, t1, env, &tp);
  if (no.why) printf("diff no %ld %s\n", no.at, no.why);
  else printf("diff ok %lld %zu\n", tp.act_delta, tp.act_ptrs.size());
  if (!no.why)
    for (size_t j = 0; j < tp.ops.size(); j++) printf("p %zu %d %lld %u\n", j, tp.ops[j].moving, tp.ops[j].delta, tp.ops[j].pshift);
}
// a window: one token's trace, launched as it is; extra_at: 0 none, else the copy that ends the window reads one byte at layer 0's raw w1 result + extra_at - 1
void window_case(const char* name, const Cfg& c, void (*tune)(RouteKnobs&, Env&) = nullptr, long long extra_at = 0) {
  const Model md(c);
  Env env;
  env.layers = c.layers, env.heads_kv = c.heads_kv;
  RouteKnobs kn;
  if (tune) tune(kn, env);
  const std::vector<RouteOp> t0 = token(c, md, 0);
  ExtraRead extra;
  if (extra_at) extra = ExtraRead{static_cast<const char*>(GemmView{t0[14]}.c()) + extra_at - 1, 1};
  printf("case %s\n", name);
  print_kinds(t0);
  print_launches(window_launches(as_plan(t0), kn, env, extra));
}

}  // namespace

int main() {
  const Cfg base;
  auto with = [&](auto f) {
    Cfg c = base;
    f(c);
    return c;
  };
  // ---- decode, one row ----
  plan_case("decode_all", base, nullptr, true);
  plan_case("decode_links_off", base, [](RouteKnobs& k, Env&) { k.links = false; });
  plan_case("decode_no_qkv_rope", base, [](RouteKnobs& k, Env&) { k.qkv_rope = false; });
  plan_case("decode_no_rope_append", base, [](RouteKnobs& k, Env&) { k.rope_append = false; });
  plan_case("decode_no_fuse", base, [](RouteKnobs& k, Env&) { k.fuse = false; });
  plan_case("decode_no_mirror", base, [](RouteKnobs&, Env& e) { e.mirrors = false; });
  plan_case("decode_kv16_off", base, [](RouteKnobs& k, Env&) { k.kv16 = false; });
  // ---- address order ----
  plan_case("order_k_first", with([](Cfg& c) { c.order = 1; }));
  plan_case("order_unequal", with([](Cfg& c) { c.v_gap = 256; }));
  plan_case("order_ldc_small", with([](Cfg& c) { c.spacing = 512; }));
  // ---- readers ----
  plan_case("reader_wo", with([](Cfg& c) { c.extra = 1; }));
  plan_case("reader_gate", with([](Cfg& c) { c.extra = 2; }));
  plan_case("reader_rewritten", with([](Cfg& c) { c.extra = 3; }));
  window_case("window_decode", base);
  window_case("window_copy_overlaps_1", base, nullptr, FF * 4);  // the last byte of the raw w1 result
  window_case("window_copy_overlaps_0", base, nullptr, FF * 4 + 1);  // the byte behind it
  // ---- shapes ----
  plan_case("shape_gqa", with([](Cfg& c) { c.heads_kv = 1; }));
  plan_case("shape_yarn", with([](Cfg& c) { c.yarn = true; }));
  plan_case("shape_k_f16", with([](Cfg& c) { c.k_f16 = true; }));
  plan_case("shape_k_f16_no_fuse", with([](Cfg& c) { c.k_f16 = true; }), [](RouteKnobs& k, Env&) { k.fuse = false; });
  plan_case("shape_n_dims", with([](Cfg& c) { c.n_dims = 64; }));
  plan_case("shape_weight_refused", base, [](RouteKnobs& k, Env& e) { k.debug = true, e.refuse = 4; });  // layer 0's w1
  // ---- prompt-sized windows ----
  window_case("prompt_16", with([](Cfg& c) { c.m = 16; }));
  window_case("prompt_17", with([](Cfg& c) { c.m = 17; }));
  window_case("prompt_17_no_norm16_scratch", with([](Cfg& c) { c.m = 17; }), [](RouteKnobs&, Env& e) { e.fail_slot = kSlotNorm16; });
  window_case("prompt_17_no_attn16_scratch", with([](Cfg& c) { c.m = 17; }), [](RouteKnobs&, Env& e) { e.fail_slot = kSlotAttn16; });
  window_case("prompt_17_no_ffn16_scratch", with([](Cfg& c) { c.m = 17; }), [](RouteKnobs&, Env& e) { e.fail_slot = kSlotFfn16; });
  window_case("prompt_17_no_table_scratch", with([](Cfg& c) { c.m = 17; }), [](RouteKnobs&, Env& e) { e.fail_slot = kSlotRopeTab; });
  window_case("prompt_17_no_mirror", with([](Cfg& c) { c.m = 17; }), [](RouteKnobs&, Env& e) { e.mirrors = false; });
  window_case("prompt_17_past_the_cache", with([](Cfg& c) { c.m = 17, c.n_past = 48; }));
  window_case("prompt_17_no_prefill_fuse", with([](Cfg& c) { c.m = 17; }), [](RouteKnobs& k, Env&) { k.prefill_fuse = false; });
  // ---- token diff ----
  diff_case("diff_two_shifts", base, base, [](std::vector<RouteOp>& t) { t[25].p[GemmView::C] = static_cast<const char*>(t[25].p[GemmView::C]) + 256; });
  diff_case("diff_field", base, base, [](std::vector<RouteOp>& t) { t[22].i[GemmView::N] += 1; });
  diff_case("diff_seq_all_still", base, base, [](std::vector<RouteOp>& t) { t[9].i[MhaView::SEQ_ALL] -= 1, t[29].i[MhaView::SEQ_ALL] -= 1; });
  diff_case("diff_mha_rows", with([](Cfg& c) { c.mha_seq = 2; }), with([](Cfg& c) { c.mha_seq = 2; }));
  diff_case("diff_foreign_write", with([](Cfg& c) { c.foreign_write = true; }), with([](Cfg& c) { c.foreign_write = true; }));
  diff_case("diff_length", base, with([](Cfg& c) { c.extra = 1; }));
  diff_case("diff_kind", base, base, [](std::vector<RouteOp>& t) { t[11].kind = RK_MUL; });
  // ---- segments: the 2-layer plan and one of about 200 launches ----
  const int segs[3][2] = {{64, 16}, {12, 6}, {1, 1}};
  for (const auto& s : segs) {
    const std::string a = "seg_small_" + std::to_string(s[0]) + "_" + std::to_string(s[1]), b = "seg_long_" + std::to_string(s[0]) + "_" + std::to_string(s[1]);
    plan_case(a.c_str(), base, nullptr, false, s[0], s[1]);
    plan_case(b.c_str(), with([](Cfg& c) { c.layers = 25; }), [](RouteKnobs& k, Env&) { k.links = false; }, false, s[0], s[1]);
    plan_case((b + "_links").c_str(), with([](Cfg& c) { c.layers = 40; }), nullptr, false, s[0], s[1]);
  }
  return 0;
}
