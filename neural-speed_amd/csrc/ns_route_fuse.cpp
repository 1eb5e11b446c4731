// ns_route_fuse.cpp — what a token's launches are: the diff of two consecutive tokens' traces (the plan), the fused launches of a plan or a window
// (ExecKind, ns_route_int.h) and the cut of a plan's launches into segments.  Pure host code: a function of the traces, the knobs and four answers
// about the device (RouteEnv).  Nothing is launched, allocated or read from the environment here — a fusion that leaves out a tensor somebody still
// reads gives wrong values, not a fault, so this file is also compiled alone and checked case by case on the host (tests/test_route_fuse.py).
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "ns_route_int.h"

namespace ns {
namespace {

using Plan = std::vector<PlanOp>;
const char* bytes_of(const void* p) { return static_cast<const char*>(p); }

// tensor `ptr` (nbytes long): is it read by any op from `from` on before somebody rewrites it, or by the copy that ends the window?
// (exact addresses: the graph's tensors are distinct allocations; a view into the middle of one would not be seen — the reference's
// llama graph has none on these tensors, and a fusion is only made from the exact node shapes that graph builds)
bool read_later(const Plan& plan, const ExtraRead& extra, const void* ptr, size_t nbytes, size_t from) {
  for (size_t j = from; j < plan.size(); j++) {
    if (is_input_of(plan[j].op, ptr)) return true;
    if (output_of(plan[j].op) == ptr) return false;
  }
  const char* c = bytes_of(ptr);
  return extra.p && c < extra.p + extra.bytes && extra.p < c + std::max<size_t>(nbytes, 1);
}
// tensor `ptr` from plan op `from` on, until somebody rewrites it: read by exactly the ops in `allowed` (all of them) and nobody else?
bool only_read_by(const Plan& plan, const void* ptr, size_t from, const int* allowed, int nallowed) {
  int seen = 0;
  for (size_t j = from; j < plan.size(); j++) {
    if (is_input_of(plan[j].op, ptr)) {
      bool ok = false;
      for (int a = 0; a < nallowed; a++) ok = ok || allowed[a] == int(j);
      if (!ok) return false;
      seen++;
    }
    if (output_of(plan[j].op) == ptr) break;
  }
  return seen == nallowed;
}
// a dense [m][n] fp32 tensor as ne hands it over (ne = {n, m, 1, 1})
bool packed_mat(const long long* ne, const long long* nb, long long n, long long m) {
  return ne[0] == n && ne[1] == m && ne[2] == 1 && ne[3] == 1 && nb[0] == 4 && (m == 1 || nb[1] == 4 * n);
}
bool packed_vec(const long long* ne, const long long* nb, long long n) { return packed_mat(ne, nb, n, 1); }
// a binary op on two dense [m][n] operands with a dense result
bool packed_binary(const BinaryView& b, long long n, long long m) {
  return packed_mat(b.ne0(), b.nb0(), n, m) && packed_mat(b.ne1(), b.nb1(), n, m) && b.nbd()[0] == 4 && (m == 1 || b.nbd()[1] == 4 * n);
}
// the same rotation: everything but the tensor and its number of heads
bool same_rope(const RouteOp& a, const RouteOp& b) {
  const RopeView x{a}, y{b};
  return a.kind == b.kind && x.batch() == y.batch() && x.seq() == y.seq() && x.head_size() == y.head_size() && x.n_past() == y.n_past() &&
         x.n_dims() == y.n_dims() && x.mode() == y.mode() && x.n_orig_ctx() == y.n_orig_ctx() && !memcmp(a.f, b.f, sizeof(a.f));
}
// the "drop dead entries" compaction of a launch list
void drop_dead(std::vector<ExecOp>& x, const std::vector<char>& dead) {
  size_t o = 0;
  for (size_t e = 0; e < x.size(); e++)
    if (!dead[e]) x[o++] = x[e];
  x.resize(o);
}
// the mul_mat ops of a launch that multiplies activations (their count; 0: not such a launch)
int gemms_of(const ExecOp& c, const Plan& plan, int gi[3]) {
  if (c.xk == XK_QKV || c.xk == XK_QKV_ROPE_M) return gi[0] = c.idx[0], gi[1] = c.idx[1], gi[2] = c.idx[2], 3;
  if (c.xk == XK_GATEUP) return gi[0] = c.idx[0], gi[1] = c.idx[2], 2;
  if (c.xk == XK_GEMM_ADD) return gi[0] = c.idx[0], 1;
  if (c.xk == XK_OP && plan[c.idx[0]].op.kind == RK_GEMM) return gi[0] = c.idx[0], 1;
  return 0;
}
// roles of the three mul_mat of a XK_QKV launch: k feeds the K cache write, v the V cache write, q is the third
struct QkvRoles {
  int q = -1, k = -1, v = -1;
  bool complete() const { return q >= 0 && k >= 0 && v >= 0; }
};
QkvRoles qkv_roles(const ExecOp& qkv, const Plan& plan, const RouteOp& dup_k, const RouteOp& dup_v) {
  QkvRoles r;
  for (int t = 0; t < 3; t++) {
    const int j = qkv.idx[t];
    const void* c = GemmView{plan[j].op}.c();
    if (c == DupView{dup_k}.src()) r.k = j;
    else if (c == DupView{dup_v}.src()) r.v = j;
    else r.q = j;
  }
  return r;
}

// ---- optimize(): the three groups that start at a mul_mat.  Each appends its launches, marks the ops it took and says whether it matched ----
struct Fuser {
  const Plan& plan;
  const RouteKnobs& kn;
  const ExtraRead& extra;
  std::vector<ExecOp> x;
  std::vector<char> used;
  int n() const { return int(plan.size()); }
  uint32_t K(int j) const { return j < n() ? plan[j].op.kind : 0u; }
  const RouteOp& O(int j) const { return plan[j].op; }
  void take(int from, int to) {
    for (int t = from; t <= to; t++) used[t] = 1;
  }
  bool qkv(int j);
  bool gateup(int j);
  bool gemm_add(int j);
};
// K, V, Q: GEMM rope dup GEMM dup GEMM rope on one input (llama.cpp:232-262 as its graph expands)
bool Fuser::qkv(int j) {
  if (!(j + 6 < n() && K(j + 1) == RK_ROPE && K(j + 2) == RK_DUP && K(j + 3) == RK_GEMM && K(j + 4) == RK_DUP && K(j + 5) == RK_GEMM && K(j + 6) == RK_ROPE))
    return false;
  const GemmView gk{O(j)}, gv{O(j + 3)}, gq{O(j + 5)};
  const RopeView rk{O(j + 1)}, rq{O(j + 6)};
  const DupView dk{O(j + 2)}, dv{O(j + 4)};
  const long long M = gk.m();
  if (!(gv.a() == gk.a() && gq.a() == gk.a() && gv.m() == M && gq.m() == M && rk.src() == gk.c() && rk.dst() == gk.c() && dk.src() == gk.c() &&
        dv.src() == gv.c() && rq.src() == gq.c() && rq.dst() == gq.c() && gk.k() == gv.k() && gk.k() == gq.k() && gk.lda() == gv.lda() && gk.lda() == gq.lda()))
    return false;
  // the three outputs in address order, equally spaced: C, C + m * ldc, C + 2 m * ldc (ip_fusion_qkv.cpp:84-86), each at least its own width
  int g[3] = {j, j + 3, j + 5};
  auto C = [&](int a) { return bytes_of(GemmView{O(g[a])}.c()); };
  for (int a = 0; a < 3; a++)
    for (int b = a + 1; b < 3; b++)
      if (C(b) < C(a)) std::swap(g[a], g[b]);
  const long long s0 = C(1) - C(0), s1 = C(2) - C(1);
  const long long ldc = s0 / (4 * M);
  bool ok = s0 == s1 && s0 % (4 * M) == 0;
  for (int a = 0; a < 3 && ok; a++) ok = ldc >= GemmView{O(g[a])}.n() && (M == 1 || GemmView{O(g[a])}.ldc() == ldc);
  if (!ok) return false;
  // rope(k) + rope(q): the q rows directly in front of the k rows (or the other way round), same parameters, one position
  const bool q_first = bytes_of(rq.src()) + rq.row_bytes() == bytes_of(rk.src());
  const bool k_first = bytes_of(rk.src()) + rk.row_bytes() == bytes_of(rq.src());
  const bool rope2 = same_rope(rk.o, rq.o) && rk.batch() == 1 && rk.seq() == 1 && (q_first || k_first);
  // ... and the two cache writes with them: plain RoPE, K handed over as packed [heads_kv][head_size] rows, fp32 cells
  const bool append = rope2 && kn.rope_append && rk.o.kind == RK_ROPE && rk.ext_factor() == 0.f && dk.ne()[0] == rk.head_size() && dk.ne()[1] == 1 &&
                      dk.ne()[2] == rk.heads() && dk.ne()[3] == 1 && dk.src_nb()[0] == 4 && dk.src_nb()[2] == rk.head_size() * 4 && !dk.dst_f16() && !dv.dst_f16();
  const int front = q_first ? j + 6 : j + 1, back = q_first ? j + 1 : j + 6;
  x.push_back(xop(XK_QKV, g[0], g[1], g[2]));
  if (append) {
    x.push_back(xop(XK_ROPE_APPEND, front, back, j + 2, j + 4));
  } else {
    if (rope2) x.push_back(xop(XK_ROPE2, front, back));
    else x.push_back(xop(XK_OP, j + 1)), x.push_back(xop(XK_OP, j + 6));
    x.push_back(xop(XK_DUP2, j + 2, j + 4));
  }
  take(j, j + 6);
  return true;
}
// gate / up: GEMM(w1) silu GEMM(w3) mul (dense rows: A [m][K], both results [m][N])
bool Fuser::gateup(int j) {
  if (!(j + 3 < n() && K(j + 1) == RK_SILU && K(j + 2) == RK_GEMM && K(j + 3) == RK_MUL)) return false;
  const GemmView g1{O(j)}, g3{O(j + 2)};
  const SiluView si{O(j + 1)};
  const BinaryView mu{O(j + 3)};
  const long long M = g1.m(), N = g1.n();
  if (!(g3.a() == g1.a() && g3.m() == M && si.src() == g1.c() && si.count() == M * N && g3.n() == N && g3.k() == g1.k() && g3.lda() == g1.lda() &&
        g1.ldc() == N && g3.ldc() == N && (M == 1 || g1.lda() == g1.k())))
    return false;
  const void *s = si.dst(), *t3 = g3.c();
  const size_t tb = size_t(M) * size_t(N) * 4;
  const bool operands = (mu.a() == s && mu.b() == t3) || (mu.a() == t3 && mu.b() == s);
  if (!(operands && packed_binary(mu, N, M) && mu.d() != s && mu.d() != t3 && !read_later(plan, extra, g1.c(), tb, j + 2) && !read_later(plan, extra, t3, tb, j + 4)))
    return false;
  x.push_back(xop(XK_GATEUP, j, j + 1, j + 2, j + 3));
  take(j, j + 3);
  return true;
}
// GEMM whose result only feeds the residual add
bool Fuser::gemm_add(int j) {
  const GemmView g{O(j)};
  if (!(j + 1 < n() && K(j + 1) == RK_ADD && g.ldc() == g.n())) return false;
  const BinaryView ad{O(j + 1)};
  const bool first = ad.a() == g.c(), second = ad.b() == g.c();
  if (!((first != second) && packed_binary(ad, g.n(), g.m()) && ad.d() != g.c() && !read_later(plan, extra, g.c(), size_t(g.m()) * size_t(g.n()) * 4, j + 2)))
    return false;
  x.push_back(xop(XK_GEMM_ADD, j, j + 1));
  take(j, j + 1);
  return true;
}
// the launches of a plan / a window, fused where the shapes allow (round 6: any row count — a prompt's window fuses like a decode step's plan,
// except the two forms that need ONE position: rope(q) + rope(k) on adjacent rows and the rope + cache-write launch)
std::vector<ExecOp> optimize(const Plan& plan, const RouteKnobs& kn, const ExtraRead& extra) {
  Fuser f{plan, kn, extra, {}, std::vector<char>(plan.size(), 0)};
  for (int j = 0; j < f.n(); j++) {
    if (f.used[j]) continue;
    const RouteOp& o = plan[j].op;
    if (kn.fuse && o.kind == RK_GEMM && GemmView{o}.m() >= 1 && (f.qkv(j) || f.gateup(j) || f.gemm_add(j))) continue;
    // a cache write outside those groups (fp32 cells): as a one-copy XK_DUP2, which keeps the fp16 mirror current under replay
    f.x.push_back(xop(o.kind == RK_DUP && !DupView{o}.dst_f16() ? XK_DUP2 : XK_OP, j));
    f.used[j] = 1;
  }
  return f.x;
}

// ---- carried RMS norms (see ExecKind): rms_norm, mul(gamma), consumer launch -> the consumer alone, if the normed tensor came out of a residual
// add that a XK_GEMM_ADD launch makes and that launch can be given the fp16 shadow of its own input.  lp->bytes: device memory asked for. ----
// On by default (NS_ROUTE_LINKS=0 or ns_hip_route_set_enabled(5) turn it off, (3) forces it on).  7B-shaped model, n_ctx 512, same box, alternating
// (profiles/r05r_route_carried_norms.txt): 323 -> 195 captured launches, GPU span per token 2009 / 1989 -> 1731 / 1737 us, 399 / 400 -> 451 / 452 tok/s.
// The carried form holds gamma . x un-normalised in fp16 (range note at ns_norm_link): an overflow shows as inf / nan, never as a wrong finite value.
size_t take_bytes(LinkPlan* lp, size_t nbytes) {
  const size_t off = lp->bytes;
  lp->bytes += (nbytes + 255) / 256 * 256;
  return off;
}
// the launch in front of producer P that can hand it its activations (the mul_mat `pg`'s input) as fp16: the attention's merge or the gate/up
// launch (itself on fp16 activations).  Returns the shadow's index, -1 with *why
int shadow_for_producer(std::vector<ExecOp>& x, const Plan& plan, int P, const GemmView& pg, LinkPlan* lp, const char** why) {
  auto O = [&](int j) -> const RouteOp& { return plan[j].op; };
  int Q = -1;
  for (int q = P - 1; q >= 0 && Q < 0; q--) {
    if (x[q].xk == XK_OP && O(x[q].idx[0]).kind == RK_MHA && MhaView{O(x[q].idx[0])}.out() == pg.a()) Q = q;
    else if (x[q].xk == XK_GATEUP && BinaryView{O(x[q].idx[3])}.d() == pg.a()) Q = q;
  }
  if (Q < 0) return *why = "no launch can hand the producer its activations as fp16", -1;
  if (x[Q].xk == XK_OP) {
    const MhaView mh{O(x[Q].idx[0])};
    if (mh.batch() != 1 || mh.seq() != 1 || mh.heads() * mh.head_size() != pg.k() || !(mh.head_size() == 64 || mh.head_size() == 128 || mh.head_size() == 256))
      return *why = "the attention in front of the producer is not a one-row decode step", -1;
  } else if (x[Q].in_link < 0 || GemmView{O(x[Q].idx[0])}.n() != pg.k()) {
    return *why = "the gate/up launch in front of the producer is not on fp16 activations itself", -1;
  }
  if (x[Q].o16 < 0) {
    lp->shadows.push_back(take_bytes(lp, size_t(pg.k()) * 2));
    x[Q].o16 = int(lp->shadows.size()) - 1;
  }
  return x[Q].o16;
}
// the norm + mul at launches e, e + 1 in front of consumer e + 2: carried (true), or why not
bool link_one(std::vector<ExecOp>& x, const Plan& plan, RouteEnv& env, LinkPlan* lp, size_t e, const char** why) {
  auto O = [&](int j) -> const RouteOp& { return plan[j].op; };
  const int jn = x[e].idx[0], jm = x[e + 1].idx[0];
  const NormView no{O(jn)};
  const BinaryView mu{O(jm)};
  const long long n = no.cols();
  const void *X = no.src(), *N = no.dst(), *N2 = mu.d();
  const bool first = mu.a() == N, second = mu.b() == N;
  if (first == second || N2 == X) return *why = "the mul does not multiply its result by a vector", false;
  const float* gamma = static_cast<const float*>(first ? mu.b() : mu.a());
  if (!packed_vec(mu.ne0(), mu.nb0(), n) || !packed_vec(mu.ne1(), mu.nb1(), n) || mu.nbd()[0] != 4) return *why = "gamma is not a dense vector of the norm's size", false;
  // ---- the consumer: every mul_mat of it reads the normed tensor, one row, K = the norm's size ----
  ExecOp& c = x[e + 2];
  int gi[3] = {-1, -1, -1};
  const int ng = gemms_of(c, plan, gi);
  if (ng == 0) return *why = "what follows is not a mul_mat launch", false;
  bool ok = c.in_link < 0;
  for (int g = 0; g < ng && ok; g++) {
    const GemmView go{O(gi[g])};
    ok = go.a() == N2 && go.m() == 1 && go.k() == n && env.weight_carries_norm(go.w());
  }
  if (!ok) return *why = "the consumer's mul_mat do not all read the normed row (one row, K = norm size, a weight the decode kernel carries norms for)", false;
  if (!only_read_by(plan, N, size_t(jn) + 1, &jm, 1) || !only_read_by(plan, N2, size_t(jm) + 1, gi, ng)) return *why = "the normed tensors have other readers", false;
  // ---- the producer: the launch whose residual add wrote the tensor that is normed ----
  int P = -1;
  for (int q = int(e) - 1; q >= 0 && P < 0; q--)
    if (x[q].xk == XK_GEMM_ADD && BinaryView{O(x[q].idx[1])}.d() == X) P = q;
  if (P < 0 || x[P].out_link >= 0) return *why = "its input is not the result of a mul_mat + add launch", false;
  const GemmView pg{O(x[P].idx[0])};
  if (pg.n() != n || pg.m() != 1 || !env.weight_carries_norm(pg.w())) return *why = "the producing mul_mat cannot carry a norm", false;
  // ... needs its own activations as fp16
  const int sh = x[P].a16 >= 0 ? x[P].a16 : shadow_for_producer(x, plan, P, pg, lp, why);
  if (sh < 0) return false;
  NormLink L;
  L.gamma = gamma, L.eps = no.eps(), L.n = int(n), L.stride = (int((n + 15) / 16) + 3) & ~3;
  L.h_off = take_bytes(lp, size_t(n) * 2), L.s_off = take_bytes(lp, size_t(L.stride) * 4);
  lp->links.push_back(L);
  const int li = int(lp->links.size()) - 1;
  x[P].out_link = li, x[P].a16 = sh;
  c.in_link = li, c.idx[XI_NORM] = jn, c.idx[XI_NORM_MUL] = jm;
  return true;
}
void link_norms(std::vector<ExecOp>& x, const Plan& plan, const RouteKnobs& kn, RouteEnv& env, LinkPlan* lp) {
  std::vector<char> dead(x.size(), 0);
  for (size_t e = 0; e + 2 < x.size(); e++) {
    if (x[e].xk != XK_OP || x[e + 1].xk != XK_OP) continue;
    const int jn = x[e].idx[0], jm = x[e + 1].idx[0];
    if (plan[jn].op.kind != RK_RMSNORM || plan[jm].op.kind != RK_MUL || NormView{plan[jn].op}.rows() != 1 || jm != jn + 1) continue;
    const char* why = nullptr;
    if (link_one(x, plan, env, lp, e, &why)) dead[e] = dead[e + 1] = 1;
    else if (kn.debug) fprintf(stderr, "route: the norm at launch %d stays a launch: %s\n", jn, why);
  }
  drop_dead(x, dead);
}

// XK_QKV (with a carried norm: its activations are an fp16 shadow) + XK_ROPE_APPEND -> XK_QKV_ROPE, one angle table per token in front (see ExecKind)
void fuse_qkv_rope(std::vector<ExecOp>& x, const Plan& plan, const RouteKnobs& kn, RouteEnv& env, LinkPlan* lp) {
  if (!kn.qkv_rope || !kn.kv16) return;
  auto O = [&](int j) -> const RouteOp& { return plan[j].op; };
  int first_rope = -1;
  std::vector<char> dead(x.size(), 0);
  for (size_t e = 0; e + 1 < x.size(); e++) {
    if (x[e].xk != XK_QKV || x[e].in_link < 0 || x[e + 1].xk != XK_ROPE_APPEND) continue;
    const ExecOp& ap = x[e + 1];
    const int jdk = ap.idx[2], jdv = ap.idx[3];
    const DupView dk{O(jdk)}, dv{O(jdv)};
    const bool k_front = dk.src() == RopeView{O(ap.idx[0])}.src();
    const int jrk = k_front ? ap.idx[0] : ap.idx[1], jrq = k_front ? ap.idx[1] : ap.idx[0];
    const RopeView rk{O(jrk)}, rq{O(jrq)};
    const QkvRoles r = qkv_roles(x[e], plan, dk.o, dv.o);
    if (!r.complete() || GemmView{O(r.q)}.c() != rq.src()) continue;
    const long long hs = rk.head_size(), hkv = rk.heads(), hq = rq.heads();
    // plain RoPE over the whole head in adjacent pairs, one position; the launch's weights as wide as the rows
    if (rk.o.kind != RK_ROPE || rk.mode() != 0 || rk.n_dims() != hs || (hs & 1) || GemmView{O(r.q)}.w()->n != hq * hs || GemmView{O(r.k)}.w()->n != hkv * hs ||
        GemmView{O(r.v)}.w()->n != hkv * hs || plan[jrk].delta != plan[jrq].delta)
      continue;
    if (first_rope >= 0 && !(same_rope(O(first_rope), rk.o) && plan[first_rope].delta == plan[jrk].delta)) continue;  // (one table serves every layer)
    KvMirrorArgs mk, mv;
    long long sd, sh;
    if (!env.mirror_of_cell(dk.dst(), &mk) || !env.mirror_of_cell(dv.dst(), &mv) || mk.transposed || !mv.transposed || mk.hs != hs || mv.hs != hs ||
        !cell_strides(dk.o, hs, hkv, &sd, &sh) || !cell_strides(dv.o, hs, hkv, &sd, &sh))
      continue;
    // the K cell's position in its cache is the RoPE position (the epilogue has one position for both)
    const long long kidx = (bytes_of(dk.dst()) - mk.base32) / 4, vidx = (bytes_of(dv.dst()) - mv.base32) / 4;
    if ((kidx / hs) % mk.n_ctx != rk.n_past() || vidx % mv.n_ctx != rk.n_past() || (kidx % hs) != 0 || plan[jdk].delta != plan[jrk].delta * hs * 4 ||
        plan[jdv].delta != plan[jrk].delta * 4)
      continue;
    if (first_rope < 0) first_rope = jrk;
    ExecOp& f = x[e];
    f.xk = XK_QKV_ROPE;
    f.idx[XI_Q] = r.q, f.idx[XI_K] = r.k, f.idx[XI_V] = r.v, f.idx[XI_ROPE_Q] = jrq, f.idx[XI_ROPE_K] = jrk, f.idx[XI_DUP_K] = jdk, f.idx[XI_DUP_V] = jdv;
    dead[e + 1] = 1;
  }
  if (first_rope < 0) return;
  lp->rope_tab_off = take_bytes(lp, size_t(RopeView{O(first_rope)}.head_size()) / 2 * 8);
  drop_dead(x, dead);
  ExecOp tab = xop(XK_ROPE_TABLE, -1);
  tab.aux = first_rope;
  x.insert(x.begin(), tab);
}

// ---- a prompt-sized window (see ExecKind): fp16 hand-overs and its two fused forms ----
// QKV + the two ropes -> the GEMM's RoPE epilogue (k / v into the kv mirror)
void prefill_qkv_rope(std::vector<ExecOp>& x, const Plan& plan, RouteEnv& env) {
  auto O = [&](int j) -> const RouteOp& { return plan[j].op; };
  std::vector<char> dead(x.size(), 0);
  for (size_t e = 0; e + 3 < x.size(); e++) {
    if (!(x[e].xk == XK_QKV && x[e + 1].xk == XK_OP && x[e + 2].xk == XK_OP && x[e + 3].xk == XK_DUP2 && x[e + 3].idx[1] >= 0)) continue;
    const int j1 = x[e + 1].idx[0], j2 = x[e + 2].idx[0], jdk = x[e + 3].idx[0], jdv = x[e + 3].idx[1];
    const RopeView r1{O(j1)}, r2{O(j2)};
    const DupView dk{O(jdk)}, dv{O(jdv)};
    const long long M = GemmView{O(x[e].idx[0])}.m();
    const QkvRoles r = qkv_roles(x[e], plan, dk.o, dv.o);
    const bool ropes = r1.o.kind == RK_ROPE && r2.o.kind == RK_ROPE && same_rope(r1.o, r2.o) && r1.in_place() && r2.in_place();
    if (!(M > 16 && ropes && r.complete())) continue;
    const bool k_is_1 = r1.src() == GemmView{O(r.k)}.c();
    const RopeView &rk = k_is_1 ? r1 : r2, &rq = k_is_1 ? r2 : r1;
    const long long hs = rk.head_size(), hkv = rk.heads(), hq = rq.heads(), np = rk.n_past();
    // plain whole-head RoPE in adjacent pairs over M consecutive positions of one sequence; K cells [head][n_ctx][hs], V cells [head][hs][n_ctx] from np on
    bool ok = rk.src() == GemmView{O(r.k)}.c() && rq.src() == GemmView{O(r.q)}.c() && rk.batch() == 1 && rk.seq() == M && rk.mode() == 0 && rk.n_dims() == hs &&
              rk.ext_factor() == 0.f && (hs & 3) == 0 && GemmView{O(r.q)}.w()->n == hq * hs && GemmView{O(r.k)}.w()->n == hkv * hs &&
              GemmView{O(r.v)}.w()->n == hkv * hs && !dk.dst_f16() && !dv.dst_f16() && dk.ne()[0] == hs && dk.ne()[1] == M && dk.ne()[2] == hkv && dk.ne()[3] == 1 &&
              dk.dst_nb()[0] == 4 && dk.dst_nb()[1] == 4 * hs && dk.dst_nb()[2] % (4 * hs) == 0 && dv.ne()[0] == M && dv.ne()[1] == hs && dv.ne()[2] == hkv &&
              dv.ne()[3] == 1 && dv.dst_nb()[0] == 4 && dv.dst_nb()[1] % 4 == 0 && dv.dst_nb()[2] == dv.dst_nb()[1] * hs;
    const long long n_ctx = ok ? dk.dst_nb()[2] / (4 * hs) : 0;
    ok = ok && n_ctx >= np + M && dv.dst_nb()[1] == 4 * n_ctx;
    _Float16 *k16 = nullptr, *v16 = nullptr;
    ok = ok && env.mirror_for_producer(bytes_of(dk.dst()) - np * hs * 4, bytes_of(dv.dst()) - np * 4, int(hkv), int(hs), int(n_ctx), int(np), int(M), &k16, &v16) &&
         env.scratch(size_t(M) * size_t(hs / 2) * 8, kSlotRopeTab) != nullptr;
    if (!ok) continue;
    ExecOp& f = x[e];
    f.xk = XK_QKV_ROPE_M;
    f.idx[XI_Q] = r.q, f.idx[XI_K] = r.k, f.idx[XI_V] = r.v, f.idx[XI_ROPE_Q] = k_is_1 ? j2 : j1, f.idx[XI_ROPE_K] = k_is_1 ? j1 : j2;
    f.idx[XI_DUP_K] = jdk, f.idx[XI_DUP_V] = jdv;  // (the cache writes stay a launch of their own: x[e + 3]; here for the mirror's geometry)
    dead[e + 1] = dead[e + 2] = 1;
  }
  drop_dead(x, dead);
}
// rms_norm + mul(gamma) at launches e, e + 1 in front of a prompt-sized mul_mat launch -> one launch, fp32 + fp16 (true: done)
bool prefill_norm16(std::vector<ExecOp>& x, const Plan& plan, RouteEnv& env, const ExtraRead& extra, size_t e) {
  auto O = [&](int j) -> const RouteOp& { return plan[j].op; };
  if (!(e + 2 < x.size() && x[e].xk == XK_OP && x[e + 1].xk == XK_OP && O(x[e].idx[0]).kind == RK_RMSNORM && O(x[e + 1].idx[0]).kind == RK_MUL)) return false;
  const int jn = x[e].idx[0], jm = x[e + 1].idx[0];
  const NormView no{O(jn)};
  const BinaryView mu{O(jm)};
  const long long rows = no.rows(), n = no.cols();
  const void *N = no.dst(), *N2 = mu.d();
  int gi[3];
  const int ng = gemms_of(x[e + 2], plan, gi);
  // (ne_mul(normed rows, gamma): the rows are the first operand, gamma the row vector — llama.cpp:178-184)
  bool ok = rows > 16 && jm == jn + 1 && mu.a() == N && mu.b() != N && N2 != no.src() && N2 != N && ng > 0 && !x[e + 2].a16p && packed_mat(mu.ne0(), mu.nb0(), n, rows) &&
            packed_vec(mu.ne1(), mu.nb1(), n) && mu.nbd()[0] == 4 && mu.nbd()[1] == 4 * n && !read_later(plan, extra, N, size_t(rows) * n * 4, size_t(jm) + 1);
  for (int g = 0; g < ng && ok; g++) {
    const GemmView go{O(gi[g])};
    ok = go.a() == N2 && go.m() == rows && go.k() == n && go.lda() == n;
  }
  void* sh = ok ? env.scratch(size_t(rows) * n * 2, kSlotNorm16) : nullptr;
  if (!sh) return false;
  x[e] = xop(XK_NORM16, jn, jm);
  x[e].o16p = sh;
  x[e + 2].a16p = sh;
  return true;
}
// the attention's rows / the gate-up product as fp16 for the projection that multiplies them
void prefill_handover(std::vector<ExecOp>& x, const Plan& plan, const RouteKnobs& kn, RouteEnv& env, size_t e) {
  auto O = [&](int j) -> const RouteOp& { return plan[j].op; };
  const RouteOp& o0 = O(x[e].idx[0]);
  const bool is_mha = x[e].xk == XK_OP && o0.kind == RK_MHA && MhaView{o0}.seq() > 16 && MhaView{o0}.batch() == 1 && kn.kv16;
  const bool is_gu = x[e].xk == XK_GATEUP && GemmView{o0}.m() > 16;
  if (!is_mha && !is_gu) return;
  const void* out = is_mha ? MhaView{o0}.out() : BinaryView{O(x[e].idx[3])}.d();
  const long long rows = is_mha ? MhaView{o0}.seq() : GemmView{o0}.m();
  const long long cols = is_mha ? MhaView{o0}.heads() * MhaView{o0}.head_size() : GemmView{o0}.n();
  for (size_t c = e + 1; c < x.size() && c < e + 4; c++) {
    int gi[3];
    if (gemms_of(x[c], plan, gi) != 1) continue;
    const GemmView go{O(gi[0])};
    if (!(go.a() == out && go.m() == rows && go.k() == cols && go.lda() == cols && !x[c].a16p)) continue;
    void* sh = env.scratch(size_t(rows) * cols * 2, is_mha ? kSlotAttn16 : kSlotFfn16);
    if (sh) x[e].o16p = sh, x[c].a16p = sh;
    return;
  }
}
void prefill_pass(std::vector<ExecOp>& x, const Plan& plan, const RouteKnobs& kn, RouteEnv& env, const ExtraRead& extra) {
  if (!kn.prefill_fuse || !kn.fuse) return;
  if (kn.kv16) prefill_qkv_rope(x, plan, env);
  std::vector<char> dead(x.size(), 0);
  for (size_t e = 0; e < x.size(); e++) {
    if (prefill_norm16(x, plan, env, extra, e)) dead[e + 1] = 1;
    else if (x[e].idx[0] >= 0) prefill_handover(x, plan, kn, env, e);
  }
  drop_dead(x, dead);
}

}  // namespace

bool cell_strides(const RouteOp& d, long long hs, long long heads_kv, long long* sd, long long* sh) {
  const DupView v{d};
  int dim_ax = -1, head_ax = -1;
  for (int ax = 0; ax < 4; ax++) {
    if (v.ne()[ax] == 1) continue;
    if (v.ne()[ax] == hs && v.src_nb()[ax] == 4 && dim_ax < 0) dim_ax = ax;
    else if (v.ne()[ax] == heads_kv && v.src_nb()[ax] == 4 * hs && head_ax < 0) head_ax = ax;
    else return false;
  }
  if (dim_ax < 0 || (heads_kv > 1 && head_ax < 0) || v.dst_f16()) return false;
  if (v.dst_nb()[dim_ax] % 4 || (head_ax >= 0 && v.dst_nb()[head_ax] % 4)) return false;
  *sd = v.dst_nb()[dim_ax] / 4, *sh = head_ax >= 0 ? v.dst_nb()[head_ax] / 4 : 0;
  return true;
}

NoPlan diff_tokens(const std::vector<RouteOp>& prev, const std::vector<RouteOp>& cur, RouteEnv& env, TokenPlan* out) {
  const size_t n = cur.size();
  if (n == 0 || n != prev.size()) return NoPlan{"the two tokens have different numbers of ops (or none)", -1, false};
  TokenPlan tp;
  tp.ops.resize(n);
  for (size_t j = 0; j < n; j++) {
    RouteOp a = prev[j];
    const RouteOp& b = cur[j];
    if (a.kind != b.kind) return NoPlan{"another operator", long(j), false};
    PlanOp po{b, 0, 0, 0u};
    // activation pointers: all shifted by ONE constant per token (the reference's device pool, see Route::act_delta)
    for (int x = 0; x < 4; x++) {
      if (x == moving_ptr(b.kind)) continue;
      const long long d = bytes_of(b.p[x]) - bytes_of(a.p[x]);
      if (d == 0) continue;
      if (tp.act_delta == 0) tp.act_delta = d;
      if (d != tp.act_delta) return NoPlan{"pointers shifted by different amounts", long(j), true};
      po.pshift |= 1u << x;
      tp.act_ptrs.insert(b.p[x]);
      a.p[x] = b.p[x];
    }
    const int mi = moving_int(b.kind), mp = moving_ptr(b.kind);
    if (mi >= 0) {  // (a value that stands still between these two tokens: delta 0, still verified every token)
      po.moving = 1, po.delta = b.i[mi] - a.i[mi];
      a.i[mi] = b.i[mi];
    }
    if (mp >= 0) {
      po.moving = 2, po.delta = bytes_of(b.p[mp]) - bytes_of(a.p[mp]);
      a.p[mp] = b.p[mp];
    }
    // something else moves: not a token loop this layer can replay
    if (memcmp(&a, &b, sizeof(RouteOp)) != 0) return NoPlan{"a field other than the moving one differs", long(j), true};
    // a moving context length is only served by the context-split attention at a decode step
    if (b.kind == RK_MHA && !(MhaView{b}.seq() == 1 && MhaView{b}.batch() == 1)) return NoPlan{"an attention over more than one row", long(j), false};
    // a plan keeps the kv mirrors current through its cache-write copies only
    KvMirrorArgs into;
    if (b.kind != RK_DUP && b.kind != RK_MHA && env.mirror_of_cell(output_of(b), &into)) return NoPlan{"an operator other than a cache write stores into a mirrored kv cache", long(j), false};
    tp.ops[j] = po;
  }
  *out = std::move(tp);
  return NoPlan{};
}

std::vector<ExecOp> plan_launches(const std::vector<PlanOp>& plan, const RouteKnobs& kn, RouteEnv& env, bool with_links, LinkPlan* lp) {
  std::vector<ExecOp> x = optimize(plan, kn, ExtraRead{});
  *lp = LinkPlan{};
  if (with_links) {
    const size_t before = x.size();
    link_norms(x, plan, kn, env, lp);
    fuse_qkv_rope(x, plan, kn, env, lp);
    if (kn.debug) fprintf(stderr, "route: %zu carried norms, %zu fp16 shadows, %zu -> %zu launches, %zu bytes\n", lp->links.size(), lp->shadows.size(), before, x.size(), lp->bytes);
  }
  return x;
}

std::vector<ExecOp> window_launches(const std::vector<PlanOp>& w, const RouteKnobs& kn, RouteEnv& env, const ExtraRead& extra) {
  std::vector<ExecOp> x = optimize(w, kn, extra);
  bool prompt_sized = false;
  for (const PlanOp& po : w) prompt_sized = prompt_sized || (po.op.kind == RK_GEMM && GemmView{po.op}.m() > 16);
  if (prompt_sized) prefill_pass(x, w, kn, env, extra);
  return x;
}

// A segment may end only where the launches so far stand for a PREFIX of the reference's launches (fusion reorders inside a layer), and never on
// a node the lazy peephole only records (a lone rms_norm or silu).  It stands for at least one of the reference's launches: it is replayed when its
// last one has matched (the angle table of XK_QKV_ROPE launches, which stands for none, is never a segment of its own).
std::vector<SegmentCut> cut_segments(const std::vector<ExecOp>& xops, const std::vector<PlanOp>& plan, const RouteKnobs& kn) {
  std::vector<SegmentCut> segs;
  std::vector<char> covered(plan.size(), 0);
  const int nx = int(xops.size());
  int ncov = 0, maxcov = -1, xbeg = 0, obeg = 0;
  for (int e = 0; e < nx; e++) {
    for (int q = 0; q < kXIdx; q++)
      if (xops[e].idx[q] >= 0 && !covered[xops[e].idx[q]]) covered[xops[e].idx[q]] = 1, ncov++, maxcov = std::max(maxcov, xops[e].idx[q]);
    const bool prefix = ncov == maxcov + 1 && maxcov + 1 > obeg;
    const uint32_t lastk = xops[e].xk == XK_OP ? plan[xops[e].idx[0]].op.kind : 0u;
    const bool enough = e + 1 - xbeg >= (segs.empty() ? kn.seg0 : kn.seg) && nx - (e + 1) >= kn.seg / 3;
    if (e + 1 == nx || (prefix && enough && lastk != RK_RMSNORM && lastk != RK_SILU)) {
      segs.push_back(SegmentCut{obeg, maxcov + 1, xbeg, e + 1});
      xbeg = e + 1, obeg = maxcov + 1;
    }
  }
  if (ncov != int(plan.size())) segs.clear();  // (cannot happen: every op is in exactly one launch)
  return segs;
}

}  // namespace ns
