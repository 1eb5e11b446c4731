// ns_route_op.h — the fields of a RouteOp (ns_common.h), stated once: which of p[4] / i[24] / f[8] holds what for each RouteKind.  The producers
// (ns_api.cpp, ns_device_load.cpp, ns_device_ops.hip, ns_device_mha.hip) fill an op through the constructors below, the route (ns_route*.cpp) reads it through the views; nobody indexes
// p / i / f by number.  The struct itself stays plain bytes: a token is verified against its plan with one memcmp per op (ns_route.cpp).
#pragma once
#include <cstddef>
#include <cstring>

#include "ns_common.h"

namespace ns {

static_assert(sizeof(RouteOp) == 264 && offsetof(RouteOp, kind) == 0 && offsetof(RouteOp, flags) == 4 && offsetof(RouteOp, p) == 8 &&
                  offsetof(RouteOp, i) == 40 && offsetof(RouteOp, f) == 232,
              "RouteOp is compared bytewise against recorded plans: its layout is fixed");

// ---- views: a RouteOp of one kind, read by name.  The enums are the indices into i[] / f[] / p[] — the one place they are written down ----
struct GemmView {  // mul_mat: C[m][n] (row stride ldc) = A[m][k] (row stride lda) . W
  enum { M, N, K, LDA, LDC };
  enum { A, W, C };
  const RouteOp& o;
  long long m() const { return o.i[M]; }
  long long n() const { return o.i[N]; }
  long long k() const { return o.i[K]; }
  long long lda() const { return o.i[LDA]; }
  long long ldc() const { return o.i[LDC]; }
  const void* a() const { return o.p[A]; }
  const ns_weight* w() const { return static_cast<const ns_weight*>(o.p[W]); }
  const void* c() const { return o.p[C]; }
};
struct BinaryView {  // add / mul: d = a (op) b, every operand with its extents and byte strides (b broadcasts)
  enum { NE0 = 0, NB0 = 4, NE1 = 8, NB1 = 12, NBD = 16 };
  enum { A, B, D };
  const RouteOp& o;
  const long long* ne0() const { return o.i + NE0; }
  const long long* nb0() const { return o.i + NB0; }
  const long long* ne1() const { return o.i + NE1; }
  const long long* nb1() const { return o.i + NB1; }
  const long long* nbd() const { return o.i + NBD; }
  const void* a() const { return o.p[A]; }
  const void* b() const { return o.p[B]; }
  const void* d() const { return o.p[D]; }
};
struct SiluView {
  enum { COUNT };
  enum { SRC, DST };
  const RouteOp& o;
  long long count() const { return o.i[COUNT]; }
  const void* src() const { return o.p[SRC]; }
  const void* dst() const { return o.p[DST]; }
};
struct NormView {
  enum { ROWS, COLS };
  enum { EPS };
  enum { SRC, DST };
  const RouteOp& o;
  long long rows() const { return o.i[ROWS]; }
  long long cols() const { return o.i[COLS]; }
  float eps() const { return o.f[EPS]; }
  const void* src() const { return o.p[SRC]; }
  const void* dst() const { return o.p[DST]; }
};
struct RopeView {  // RK_ROPE and RK_ROPE_YARN (which also has n_orig_ctx, beta_fast, beta_slow)
  enum { BATCH, SEQ, HEADS, HEAD_SIZE, N_PAST, N_DIMS, MODE, N_ORIG_CTX };
  enum { FREQ_BASE, FREQ_SCALE, EXT_FACTOR, ATTN_FACTOR, BETA_FAST, BETA_SLOW };
  enum { SRC, DST };
  const RouteOp& o;
  long long batch() const { return o.i[BATCH]; }
  long long seq() const { return o.i[SEQ]; }
  long long heads() const { return o.i[HEADS]; }
  long long head_size() const { return o.i[HEAD_SIZE]; }
  long long n_past() const { return o.i[N_PAST]; }
  long long n_dims() const { return o.i[N_DIMS]; }
  long long mode() const { return o.i[MODE]; }
  long long n_orig_ctx() const { return o.i[N_ORIG_CTX]; }
  float freq_base() const { return o.f[FREQ_BASE]; }
  float freq_scale() const { return o.f[FREQ_SCALE]; }
  float ext_factor() const { return o.f[EXT_FACTOR]; }
  float attn_factor() const { return o.f[ATTN_FACTOR]; }
  float beta_fast() const { return o.f[BETA_FAST]; }
  float beta_slow() const { return o.f[BETA_SLOW]; }
  const void* src() const { return o.p[SRC]; }
  const void* dst() const { return o.p[DST]; }
  bool in_place() const { return src() == dst(); }
  long long row_bytes() const { return heads() * head_size() * 4; }  // one position's rows
};
struct DupView {  // cpy: the destination (a kv-cache cell under replay) may be fp16
  enum { NE = 0, SRC_NB = 4, DST_NB = 8, DST_F16 = 12 };
  enum { SRC, DST };
  const RouteOp& o;
  const long long* ne() const { return o.i + NE; }
  const long long* src_nb() const { return o.i + SRC_NB; }
  const long long* dst_nb() const { return o.i + DST_NB; }
  bool dst_f16() const { return o.i[DST_F16] != 0; }
  const void* src() const { return o.p[SRC]; }
  const void* dst() const { return o.p[DST]; }
};
struct MhaView {  // the device-layout attention: K [batch][heads_kv][n_ctx][head_size], V transposed
  enum { BATCH, SEQ, SEQ_ALL, HEADS, HEADS_KV, HEAD_SIZE, N_CTX, MASKED };
  enum { SCALE };
  enum { Q, K, V, OUT };
  const RouteOp& o;
  long long batch() const { return o.i[BATCH]; }
  long long seq() const { return o.i[SEQ]; }
  long long seq_all() const { return o.i[SEQ_ALL]; }
  long long heads() const { return o.i[HEADS]; }
  long long heads_kv() const { return o.i[HEADS_KV]; }
  long long head_size() const { return o.i[HEAD_SIZE]; }
  long long n_ctx() const { return o.i[N_CTX]; }
  long long masked() const { return o.i[MASKED]; }
  float scale() const { return o.f[SCALE]; }
  const void* q() const { return o.p[Q]; }
  const void* k() const { return o.p[K]; }
  const void* v() const { return o.p[V]; }
  const void* out() const { return o.p[OUT]; }
};

// ---- constructors: zero-initialised (the padding too: ops are compared bytewise), then filled ----
inline RouteOp route_op_zero(uint32_t kind) {
  RouteOp op;
  memset(&op, 0, sizeof(op));
  op.kind = kind;
  return op;
}
inline RouteOp route_op_gemm(const void* a, const ns_weight* w, void* c, long long m, long long n, long long k, long long lda, long long ldc) {
  RouteOp op = route_op_zero(RK_GEMM);
  op.p[GemmView::A] = a, op.p[GemmView::W] = w, op.p[GemmView::C] = c;
  op.i[GemmView::M] = m, op.i[GemmView::N] = n, op.i[GemmView::K] = k, op.i[GemmView::LDA] = lda, op.i[GemmView::LDC] = ldc;
  return op;
}
inline RouteOp route_op_binary(uint32_t kind, const void* a, const void* b, void* d, const long long ne0[4], const long long nb0[4], const long long ne1[4],
                               const long long nb1[4], const long long nbd[4]) {  // kind: RK_ADD or RK_MUL
  RouteOp op = route_op_zero(kind);
  op.p[BinaryView::A] = a, op.p[BinaryView::B] = b, op.p[BinaryView::D] = d;
  for (int x = 0; x < 4; x++)
    op.i[BinaryView::NE0 + x] = ne0[x], op.i[BinaryView::NB0 + x] = nb0[x], op.i[BinaryView::NE1 + x] = ne1[x], op.i[BinaryView::NB1 + x] = nb1[x],
                           op.i[BinaryView::NBD + x] = nbd[x];
  return op;
}
inline RouteOp route_op_silu(const void* src, void* dst, long long count) {
  RouteOp op = route_op_zero(RK_SILU);
  op.p[SiluView::SRC] = src, op.p[SiluView::DST] = dst, op.i[SiluView::COUNT] = count;
  return op;
}
inline RouteOp route_op_rms_norm(const void* src, void* dst, long long rows, long long cols, float eps) {
  RouteOp op = route_op_zero(RK_RMSNORM);
  op.p[NormView::SRC] = src, op.p[NormView::DST] = dst, op.i[NormView::ROWS] = rows, op.i[NormView::COLS] = cols, op.f[NormView::EPS] = eps;
  return op;
}
inline RouteOp route_op_rope(const void* src, void* dst, long long batch, long long seq, long long heads, long long head_size, long long n_past, long long n_dims,
                             long long mode, float freq_base, float freq_scale, float ext_factor, float attn_factor) {
  RouteOp op = route_op_zero(RK_ROPE);
  op.p[RopeView::SRC] = src, op.p[RopeView::DST] = dst;
  op.i[RopeView::BATCH] = batch, op.i[RopeView::SEQ] = seq, op.i[RopeView::HEADS] = heads, op.i[RopeView::HEAD_SIZE] = head_size, op.i[RopeView::N_PAST] = n_past,
  op.i[RopeView::N_DIMS] = n_dims, op.i[RopeView::MODE] = mode;
  op.f[RopeView::FREQ_BASE] = freq_base, op.f[RopeView::FREQ_SCALE] = freq_scale, op.f[RopeView::EXT_FACTOR] = ext_factor, op.f[RopeView::ATTN_FACTOR] = attn_factor;
  return op;
}
inline RouteOp route_op_rope_yarn(const void* src, void* dst, long long batch, long long seq, long long heads, long long head_size, long long n_past,
                                  long long n_dims, long long mode, float freq_base, float freq_scale, long long n_orig_ctx, float ext_factor, float attn_factor,
                                  float beta_fast, float beta_slow) {
  RouteOp op = route_op_rope(src, dst, batch, seq, heads, head_size, n_past, n_dims, mode, freq_base, freq_scale, ext_factor, attn_factor);
  op.kind = RK_ROPE_YARN;
  op.i[RopeView::N_ORIG_CTX] = n_orig_ctx, op.f[RopeView::BETA_FAST] = beta_fast, op.f[RopeView::BETA_SLOW] = beta_slow;
  return op;
}
inline RouteOp route_op_dup(const void* src, void* dst, const long long ne[4], const long long src_nb[4], const long long dst_nb[4], bool dst_f16) {
  RouteOp op = route_op_zero(RK_DUP);
  op.p[DupView::SRC] = src, op.p[DupView::DST] = dst;
  for (int x = 0; x < 4; x++) op.i[DupView::NE + x] = ne[x], op.i[DupView::SRC_NB + x] = src_nb[x], op.i[DupView::DST_NB + x] = dst_nb[x];
  op.i[DupView::DST_F16] = dst_f16 ? 1 : 0;
  return op;
}
inline RouteOp route_op_mha(const void* q, const void* k, const void* v, void* out, long long batch, long long seq, long long seq_all, long long heads,
                            long long heads_kv, long long head_size, long long n_ctx, float scale, long long masked) {
  RouteOp op = route_op_zero(RK_MHA);
  op.p[MhaView::Q] = q, op.p[MhaView::K] = k, op.p[MhaView::V] = v, op.p[MhaView::OUT] = out;
  op.i[MhaView::BATCH] = batch, op.i[MhaView::SEQ] = seq, op.i[MhaView::SEQ_ALL] = seq_all, op.i[MhaView::HEADS] = heads, op.i[MhaView::HEADS_KV] = heads_kv,
  op.i[MhaView::HEAD_SIZE] = head_size, op.i[MhaView::N_CTX] = n_ctx, op.i[MhaView::MASKED] = masked;
  op.f[MhaView::SCALE] = scale;
  return op;
}

// ---- what the route asks of an op whatever its kind ----
// the one integer field of a kind that may move from token to token (index into RouteOp::i), -1: none
inline int moving_int(uint32_t kind) {
  switch (kind) {
    case RK_ROPE:
    case RK_ROPE_YARN: return RopeView::N_PAST;
    case RK_MHA: return MhaView::SEQ_ALL;
    default: return -1;
  }
}
// the one pointer of a kind that may move (index into RouteOp::p), -1: none — a cache write's destination (a kv-cache cell)
inline int moving_ptr(uint32_t kind) { return kind == RK_DUP ? int(DupView::DST) : -1; }
inline bool is_input_of(const RouteOp& o, const void* ptr) {
  switch (o.kind) {
    case RK_GEMM: return GemmView{o}.a() == ptr;
    case RK_ADD:
    case RK_MUL: return BinaryView{o}.a() == ptr || BinaryView{o}.b() == ptr;
    case RK_MHA: return MhaView{o}.q() == ptr || MhaView{o}.k() == ptr || MhaView{o}.v() == ptr;
    default: return o.p[0] == ptr;  // silu, norm, rope (in place: also its output), dup: all have their source first
  }
}
inline const void* output_of(const RouteOp& o) {
  switch (o.kind) {
    case RK_GEMM: return GemmView{o}.c();
    case RK_ADD:
    case RK_MUL: return BinaryView{o}.d();
    case RK_MHA: return MhaView{o}.out();
    default: return o.p[1];  // silu, norm, rope, dup: all have their destination second
  }
}
static_assert(SiluView::SRC == 0 && NormView::SRC == 0 && RopeView::SRC == 0 && DupView::SRC == 0 && SiluView::DST == 1 && NormView::DST == 1 &&
                  RopeView::DST == 1 && DupView::DST == 1,
              "is_input_of / output_of read the unary kinds' source and destination at p[0] / p[1]");

}  // namespace ns
