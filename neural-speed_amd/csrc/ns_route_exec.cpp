// ns_route_exec.cpp — issuing one launch of the device route: an operator as the reference asked for it (execute), or one of the fused launches the
// planner made of a plan's or a window's ops (issue_launch: one function per ExecKind, ns_route_int.h).  Inside a plan's stream capture the device
// counter kdev moves what moves per token (g_affine, g_kvm); a window launches plain values (kdev == nullptr).
#include <hip/hip_runtime.h>

#include "../../include/ns_bestla.h"
#include "ns_common.h"
#include "ns_route_int.h"

namespace ns {
// what a launch issued here is told beside its arguments (ns_common.h, ns_route.h): set around the call, cleared behind it (ExecGuard)
thread_local Affine g_affine;
thread_local void* g_mha_out16 = nullptr;
thread_local bool g_mha_out16_written = false;
thread_local KvMirrorPair g_kvm;
namespace {

thread_local bool t_in_exec = false;

const float* F(const void* p) { return static_cast<const float*>(p); }
float* M(const void* p) { return static_cast<float*>(const_cast<void*>(p)); }
void* V(const void* p) { return const_cast<void*>(p); }
int fail(const char* what) {
  set_error(what);
  return -1;
}

// one launch being issued: the plan ops it stands for, by slot of ExecOp::idx
struct Issue {
  const ExecOp& xo;
  const std::vector<PlanOp>& plan;
  const LinkMem& lm;
  const int* kdev;
  hipStream_t st;
  const PlanOp& P(int slot) const { return plan[xo.idx[slot]]; }
  const RouteOp& O(int slot) const { return P(slot).op; }
  // a captured cache write also stores into the fp16 mirror of the cache it writes (ns_route.h); a window's attention converts what it needs itself
  void mirror_of(const void* cell, KvMirrorArgs* out) const {
    if (kdev && kv16_enabled()) (void)kvm_args_for_cell(cell, out);
  }
  const NormLink& link(int li) const { return lm.lp->links[li]; }
  void* link_h(int li) const { return lm.mem + link(li).h_off; }  // fp16(gamma . x) of a carried norm
  void* shadow(int si) const { return si >= 0 ? lm.mem + lm.lp->shadows[si] : nullptr; }
  float* rope_table() const { return reinterpret_cast<float*>(lm.mem + lm.lp->rope_tab_off); }
  ns_norm_link in_link() const {  // the consumer side of a carried norm
    const NormLink& L = link(xo.in_link);
    ns_norm_link lk{};
    lk.in_ssq = reinterpret_cast<const float*>(lm.mem + L.s_off), lk.in_parts = (L.n + 15) / 16, lk.in_stride = L.stride, lk.eps = L.eps, lk.norm_size = L.n;
    return lk;
  }
};

// what the RoPE epilogue of both fused QKV launches is told: plain whole-head RoPE from an angle table, k / v rows into the fp16 mirror
ns_qkv_rope qkv_rope_args(const RopeView& rq, const RopeView& rk, _Float16* k16, _Float16* v16, const float* table, long long n_ctx) {
  ns_qkv_rope r{};
  r.kcache16 = k16, r.vcache16 = v16, r.cos_sin = table;
  r.heads = int(rq.heads()), r.heads_kv = int(rk.heads()), r.head_size = int(rk.head_size()), r.n_past = int(rk.n_past()), r.n_dims = int(rk.n_dims()), r.mode = 0;
  r.cache_step_sl = rk.head_size(), r.cache_step_head = n_ctx * rk.head_size(), r.flags = 0;
  return r;
}

int issue_norm16(const Issue& s) {
  const NormView no{s.O(0)};
  const BinaryView mu{s.O(1)};
  return ns_hip_norm_mul_h(int(no.rows()), int(no.cols()), true, no.eps(), F(no.src()), F(mu.b()), M(mu.d()), s.xo.o16p, s.st);
}
int issue_qkv_rope_m(const Issue& s) {
  const GemmView gq{s.O(XI_Q)}, gk{s.O(XI_K)}, gv{s.O(XI_V)};
  const RopeView rq{s.O(XI_ROPE_Q)}, rk{s.O(XI_ROPE_K)};
  const DupView dk{s.O(XI_DUP_K)}, dv{s.O(XI_DUP_V)};
  const long long hs = rk.head_size(), np = rk.n_past(), m = gq.m(), n_ctx = dk.dst_nb()[2] / (4 * hs);
  _Float16 *k16 = nullptr, *v16 = nullptr;
  float* tab = static_cast<float*>(stream_scratch(s.st, size_t(m) * size_t(hs / 2) * 8, kSlotRopeTab));
  int rc = -2;
  if (tab && kvm_for_producer(static_cast<const char*>(dk.dst()) - np * hs * 4, static_cast<const char*>(dv.dst()) - np * 4, int(rk.heads()), int(hs), int(n_ctx),
                              int(np), int(m), &k16, &v16) &&
      launch_rope_cos_sin(int(m), int(np), int(rk.n_dims()), rk.freq_base(), rk.freq_scale(), rk.attn_factor(), tab, s.st) == hipSuccess) {
    const ns_qkv_rope r = qkv_rope_args(rq, rk, k16, v16, tab, n_ctx);
    rc = qkv_rope_route_forward_m(F(gq.a()), s.xo.a16p, gq.w(), gk.w(), gv.w(), M(gq.c()), M(gk.c()), M(gv.c()), int(m), int(gq.lda()), int(gq.ldc()), &r, s.st);
  }
  if (rc != -2) return rc;
  kvm_note_foreign_write(dk.dst(), 1);  // (nothing was stored into the mirror after all: it starts over)
  // the GEMM does not take this shape: the three mul_mat in one launch and the two ropes, as the window had them (the mirror's rows are converted by the attention)
  ns_hip_reset_error();
  for (const GemmView* g : {&gq, &gk, &gv})
    if (ns_hip_f32f32_forward_h(F(g->a()), s.xo.a16p, g->w(), M(g->c()), nullptr, int(m), int(g->lda()), int(gq.ldc()), NS_EPI_NONE, nullptr, 0, s.st) != 0) return -1;
  if (execute(rk.o, s.st) != 0) return -1;
  return execute(rq.o, s.st);
}
int issue_rope_table(const Issue& s) {
  const PlanOp& po = s.plan[s.xo.aux];
  const RopeView r{po.op};
  g_affine = Affine{s.kdev, po.delta, 0};
  if (launch_rope_cos_sin(1, int(r.n_past()), int(r.n_dims()), r.freq_base(), r.freq_scale(), r.attn_factor(), s.rope_table(), s.st) != hipSuccess)
    return fail("device route: rope table launch failed");
  return 0;
}
int issue_qkv_rope(const Issue& s) {
  const GemmView gq{s.O(XI_Q)}, gk{s.O(XI_K)}, gv{s.O(XI_V)};
  const RopeView rq{s.O(XI_ROPE_Q)}, rk{s.O(XI_ROPE_K)};
  const DupView dk{s.O(XI_DUP_K)}, dv{s.O(XI_DUP_V)};
  KvMirrorArgs mk, mv;
  if (!kvm_args_for_cell(dk.dst(), &mk) || !kvm_args_for_cell(dv.dst(), &mv)) return fail("device route: the kv mirror of a fused QKV launch is gone");
  const long long hs = rk.head_size(), hkv = rk.heads();
  const long long kidx = (static_cast<const char*>(dk.dst()) - mk.base32) / 4, per_slot = hkv * mk.n_ctx * hs;
  const long long slot = kidx / per_slot;
  const ns_qkv_rope r = qkv_rope_args(rq, rk, mk.m16 + slot * per_slot, mv.m16 + slot * per_slot, s.rope_table(), mk.n_ctx);
  QkvRopeRoute rr{};
  rr.k32 = M(dk.dst()), rr.v32 = M(dv.dst());
  if (!cell_strides(dk.o, hs, hkv, &rr.k32_dim, &rr.k32_head) || !cell_strides(dv.o, hs, hkv, &rr.v32_dim, &rr.v32_head)) return -1;
  rr.k32_tok = s.P(XI_DUP_K).delta / 4, rr.v32_tok = s.P(XI_DUP_V).delta / 4;
  rr.kmove = s.kdev, rr.kd_pos = int(s.P(XI_ROPE_K).delta);
  rr.overflow = kvm_overflow_word();
  const ns_norm_link lk = s.in_link();
  return qkv_rope_route_forward(F(gq.a()), s.link_h(s.xo.in_link), gq.w(), gk.w(), gv.w(), M(gq.c()), M(gk.c()), M(gv.c()), int(gq.lda()), &lk, &r, &rr, s.st);
}
int issue_qkv(const Issue& s) {  // the three mul_mat in address order of their outputs
  const GemmView a{s.O(0)}, b{s.O(1)}, c{s.O(2)};
  const int m = int(a.m());
  const long long ldc = (static_cast<const char*>(b.c()) - static_cast<const char*>(a.c())) / (4 * m);
  if (s.xo.in_link >= 0) {
    const ns_norm_link lk = s.in_link();
    return ns_hip_fusion_qkv_forward_x(F(a.a()), s.link_h(s.xo.in_link), a.w(), b.w(), c.w(), M(a.c()), nullptr, 1, int(a.lda()), int(ldc), &lk, s.st);
  }
  if (s.xo.a16p) return ns_hip_fusion_qkv_forward_h(F(a.a()), s.xo.a16p, a.w(), b.w(), c.w(), M(a.c()), nullptr, m, int(a.lda()), int(ldc), s.st);
  return ns_hip_fusion_qkv_forward(F(a.a()), a.w(), b.w(), c.w(), M(a.c()), m, int(a.lda()), int(ldc), s.st);
}
int issue_rope2(const Issue& s) {
  const RopeView a{s.O(0)}, b{s.O(1)};  // a: the rows in front; the other tensor's rows follow directly
  g_affine = Affine{s.kdev, s.P(0).delta, 0};
  const int heads = int(a.heads() + b.heads());
  if (a.o.kind == RK_ROPE_YARN)
    return ns_hip_rope_f32_yarn(F(a.src()), M(a.dst()), 1, 1, heads, int(a.head_size()), int(a.n_past()), int(a.n_dims()), int(a.mode()), a.freq_base(), a.freq_scale(),
                                int(a.n_orig_ctx()), a.ext_factor(), a.attn_factor(), a.beta_fast(), a.beta_slow(), s.st);
  return ns_hip_rope_f32(F(a.src()), M(a.dst()), 1, 1, heads, int(a.head_size()), int(a.n_past()), int(a.n_dims()), int(a.mode()), a.freq_base(), a.freq_scale(),
                         a.ext_factor(), a.attn_factor(), s.st);
}
int issue_rope_append(const Issue& s) {
  const RopeView a{s.O(0)}, b{s.O(1)};  // a: the rope whose rows come first
  const DupView dk{s.O(2)}, dv{s.O(3)};  // the cache writes
  const bool k_is_front = dk.src() == a.src();
  const RopeView& rk = k_is_front ? a : b;
  g_affine = Affine{s.kdev, s.P(0).delta, 0};
  s.mirror_of(dk.dst(), &g_kvm.k), s.mirror_of(dv.dst(), &g_kvm.v);
  if (launch_rope_append(M(a.src()), int(a.heads() + b.heads()), k_is_front ? 0 : int(a.heads()), int(rk.heads()), int(a.head_size()), int(a.n_past()), int(a.n_dims()),
                         int(a.mode()), a.freq_base(), a.freq_scale(), a.attn_factor(), 0.f, 0.f, 0.f, dk.src(), V(dk.dst()), dk.ne(), dk.src_nb(), dk.dst_nb(), dv.src(),
                         V(dv.dst()), dv.ne(), dv.src_nb(), dv.dst_nb(), s.P(2).delta, s.P(3).delta, s.st) != hipSuccess)
    return fail("device route: rope + kv-cache write launch failed");
  return 0;
}
int issue_dup2(const Issue& s) {
  const DupView a{s.O(0)};
  static const long long none[4] = {0, 0, 0, 0};
  hipError_t e;
  if (s.xo.idx[1] < 0) {  // one cache write on its own
    g_affine = Affine{s.kdev, s.P(0).delta, 0};
    s.mirror_of(a.dst(), &g_kvm.k);
    e = launch_dup2(a.src(), V(a.dst()), a.ne(), a.src_nb(), a.dst_nb(), a.dst_f16(), a.src(), V(a.dst()), none, none, none, false, s.st);
  } else {
    const DupView b{s.O(1)};
    g_affine = Affine{s.kdev, s.P(0).delta, s.P(1).delta};
    if (!a.dst_f16()) s.mirror_of(a.dst(), &g_kvm.k);
    if (!b.dst_f16()) s.mirror_of(b.dst(), &g_kvm.v);
    e = launch_dup2(a.src(), V(a.dst()), a.ne(), a.src_nb(), a.dst_nb(), a.dst_f16(), b.src(), V(b.dst()), b.ne(), b.src_nb(), b.dst_nb(), b.dst_f16(), s.st);
  }
  return e == hipSuccess ? 0 : fail("device route: kv-cache write launch failed");
}
int issue_gemm_add(const Issue& s) {
  const GemmView g{s.O(0)};
  const BinaryView ad{s.O(1)};
  const ExecOp& xo = s.xo;
  const void* other = ad.a() == g.c() ? ad.b() : ad.a();
  const int n = int(g.n());
  if (xo.in_link >= 0 || xo.out_link >= 0) {
    ns_norm_link lk = xo.in_link >= 0 ? s.in_link() : ns_norm_link{};
    void* c16 = nullptr;
    if (xo.out_link >= 0) {
      const NormLink& L = s.link(xo.out_link);
      lk.out_gamma = L.gamma, lk.out_ssq = reinterpret_cast<float*>(s.lm.mem + L.s_off), lk.out_stride = L.stride;
      c16 = s.link_h(xo.out_link);
    }
    const void* a16 = xo.in_link >= 0 ? s.link_h(xo.in_link) : s.shadow(xo.a16);
    return ns_hip_f32f32_forward_x(F(g.a()), a16, g.w(), M(ad.d()), c16, 1, int(g.lda()), n, NS_EPI_ADD, F(other), n, &lk, s.st);
  }
  if (xo.a16p) return ns_hip_f32f32_forward_h(F(g.a()), xo.a16p, g.w(), M(ad.d()), nullptr, int(g.m()), int(g.lda()), n, NS_EPI_ADD, F(other), n, s.st);
  return ns_hip_f32f32_forward(F(g.a()), g.w(), M(ad.d()), int(g.m()), int(g.lda()), n, NS_EPI_ADD, F(other), n, s.st);
}
int issue_gateup(const Issue& s) {
  const GemmView g1{s.O(0)}, g3{s.O(2)};
  const SiluView si{s.O(1)};
  const BinaryView mu{s.O(3)};
  const ExecOp& xo = s.xo;
  if (xo.in_link >= 0) {
    const ns_norm_link lk = s.in_link();
    return ns_hip_fusion_ffn3_gateup_x(F(g1.a()), s.link_h(xo.in_link), g1.w(), g3.w(), M(si.dst()), M(mu.d()), s.shadow(xo.o16), 1, NS_EPI_SILU, &lk, s.st);
  }
  if (xo.a16p || xo.o16p) return ns_hip_fusion_ffn3_gateup_x(F(g1.a()), xo.a16p, g1.w(), g3.w(), M(si.dst()), M(mu.d()), xo.o16p, int(g1.m()), NS_EPI_SILU, nullptr, s.st);
  return ns_hip_fusion_ffn3_gateup(F(g1.a()), g1.w(), g3.w(), M(si.dst()), M(mu.d()), int(g1.m()), NS_EPI_SILU, s.st);
}
int issue_op(const Issue& s) {  // one operator of the reference's
  const PlanOp& po = s.P(0);
  const ExecOp& xo = s.xo;
  if (po.op.kind == RK_GEMM && (xo.in_link >= 0 || xo.a16p)) {
    const GemmView g{po.op};
    if (xo.in_link >= 0) {  // (the model's last norm in front of the output projection)
      const ns_norm_link lk = s.in_link();
      return ns_hip_f32f32_forward_x(F(g.a()), s.link_h(xo.in_link), g.w(), M(g.c()), nullptr, int(g.m()), int(g.lda()), int(g.ldc()), NS_EPI_NONE, nullptr, 0, &lk, s.st);
    }
    // (a window's prompt-sized projection on the fp16 rows its producer left)
    return ns_hip_f32f32_forward_h(F(g.a()), xo.a16p, g.w(), M(g.c()), nullptr, int(g.m()), int(g.lda()), int(g.ldc()), NS_EPI_NONE, nullptr, 0, s.st);
  }
  if (po.moving) g_affine = Affine{s.kdev, po.delta, 0};
  if (xo.o16 >= 0 && po.op.kind == RK_MHA) g_mha_out16 = s.shadow(xo.o16);
  if (xo.o16p && po.op.kind == RK_MHA) g_mha_out16 = xo.o16p;
  const int rc = execute(po.op, s.st);
  g_mha_out16 = nullptr;
  return rc;
}

}  // namespace

ExecGuard::ExecGuard() : was_(t_in_exec) { t_in_exec = true; }
ExecGuard::~ExecGuard() {
  t_in_exec = was_;
  if (!was_) g_affine = Affine{}, g_kvm = KvMirrorPair{};
}
bool route_executing() { return t_in_exec; }

int flush_lazy_node() {
  ExecGuard guard;
  return ns_hip_lazy_flush();
}

int execute(const RouteOp& op, hipStream_t st) {
  ExecGuard guard;
  // the glue launches a recorded norm / silu node before anything that is not its fusable consumer (ne_bestla_hip_device.c): the same here
  if (op.kind != RK_MUL && op.kind != RK_RMSNORM && op.kind != RK_SILU && ns_hip_lazy_flush() != 0) return -1;
  // an operator other than the cache-write copy that stores into a mirrored kv cache (an in-place shift): the mirror starts over
  if (op.kind != RK_DUP && op.kind != RK_MHA) kvm_note_foreign_write(output_of(op), 1);
  switch (op.kind) {
    case RK_GEMM: {
      const GemmView g{op};
      return ns_hip_f32f32_forward(F(g.a()), g.w(), M(g.c()), int(g.m()), int(g.lda()), int(g.ldc()), NS_EPI_NONE, nullptr, 0, st);
    }
    case RK_ADD:
    case RK_MUL: {
      const BinaryView b{op};
      if (op.kind == RK_ADD) return ns_hip_binary_nd_f32(0, F(b.a()), F(b.b()), M(b.d()), b.ne0(), b.nb0(), b.ne1(), b.nb1(), b.nbd(), st);
      return ns_hip_lazy_mul(F(b.a()), F(b.b()), M(b.d()), b.ne0(), b.nb0(), b.ne1(), b.nb1(), b.nbd(), st);
    }
    case RK_SILU: {
      const SiluView s{op};
      return ns_hip_lazy_silu(F(s.src()), M(s.dst()), size_t(s.count()), st);
    }
    case RK_RMSNORM: {
      const NormView n{op};
      return ns_hip_lazy_rms_norm(int(n.rows()), int(n.cols()), n.eps(), F(n.src()), M(n.dst()), st);
    }
    case RK_ROPE: {
      const RopeView r{op};
      return ns_hip_rope_f32(F(r.src()), M(r.dst()), int(r.batch()), int(r.seq()), int(r.heads()), int(r.head_size()), int(r.n_past()), int(r.n_dims()), int(r.mode()),
                             r.freq_base(), r.freq_scale(), r.ext_factor(), r.attn_factor(), st);
    }
    case RK_ROPE_YARN: {
      const RopeView r{op};
      return ns_hip_rope_f32_yarn(F(r.src()), M(r.dst()), int(r.batch()), int(r.seq()), int(r.heads()), int(r.head_size()), int(r.n_past()), int(r.n_dims()),
                                  int(r.mode()), r.freq_base(), r.freq_scale(), int(r.n_orig_ctx()), r.ext_factor(), r.attn_factor(), r.beta_fast(), r.beta_slow(), st);
    }
    case RK_DUP: {
      const DupView d{op};
      return ns_hip_dup_f32(F(d.src()), V(d.dst()), d.ne(), d.src_nb(), d.dst_nb(), d.dst_f16(), st);
    }
    case RK_MHA: {
      const MhaView a{op};
      return ns_hip_mha_f32_device_layout(F(a.q()), F(a.k()), F(a.v()), M(a.out()), int(a.batch()), int(a.seq()), int(a.seq_all()), int(a.heads()), int(a.heads_kv()),
                                          int(a.head_size()), int(a.n_ctx()), a.scale(), int(a.masked()), st);
    }
    default: return fail("device route: unknown operator in the plan");
  }
}

int issue_launch(const ExecOp& xo, const std::vector<PlanOp>& plan, const LinkMem& lm, const int* kdev, hipStream_t st) {
  ExecGuard guard;
  if (xo.xk != XK_OP && ns_hip_lazy_flush() != 0) return -1;
  const Issue s{xo, plan, lm, kdev, st};
  switch (xo.xk) {
    case XK_NORM16: return issue_norm16(s);
    case XK_QKV_ROPE_M: return issue_qkv_rope_m(s);
    case XK_ROPE_TABLE: return issue_rope_table(s);
    case XK_QKV_ROPE: return issue_qkv_rope(s);
    case XK_QKV: return issue_qkv(s);
    case XK_ROPE2: return issue_rope2(s);
    case XK_ROPE_APPEND: return issue_rope_append(s);
    case XK_DUP2: return issue_dup2(s);
    case XK_GEMM_ADD: return issue_gemm_add(s);
    case XK_GATEUP: return issue_gateup(s);
    default: return issue_op(s);
  }
}

}  // namespace ns
