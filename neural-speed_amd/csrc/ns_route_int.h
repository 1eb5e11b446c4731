// ns_route_int.h — what the three files of the device route share (internal; the entry points are in ns_common.h / ns_route.h):
//   ns_route_fuse.cpp  decides what a token's launches are: pure host code over op traces (tests/test_route_fuse.py runs it without a device)
//   ns_route_exec.cpp  issues one launch
//   ns_route.cpp       the per-queue state machine: window, plans, capture, replay
#pragma once
#include <cstdint>
#include <unordered_set>
#include <vector>

#include "ns_route.h"
#include "ns_route_op.h"

namespace ns {

struct PlanOp {
  RouteOp op;       // the values of the token the plan was made from (k = 0)
  int moving;       // 0 nothing moves, 1 the integer field moving_int(kind), 2 the pointer moving_ptr(kind)
  long long delta;  // per token
  unsigned pshift;  // bit x: pointer p[x] is an ACTIVATION of the reference's device pool — it arrives shifted by TokenPlan::act_delta per token
                    // (Route::act_delta, ns_route.cpp) and is replayed at the plan's address
};
// What a segment's graph actually launches.  The reference builds its decode graph from single operators (llama.cpp:203-330: rms_norm,
// mul, three mul_mat, two rope, two cpy, flash_attn, mul_mat, add, ...); a plan knows the whole token, so at capture time runs of them
// become the library's fused launches — same tensors written, same values (the reference's own fused nodes compute exactly these):
//   XK_QKV      three mul_mat of one input, outputs equally spaced   -> ns_hip_fusion_qkv_forward       (ip_fusion_qkv.cpp:84-86)
//   XK_ROPE2    rope(q) and rope(k) in place on adjacent rows         -> one rope launch over both
//   XK_DUP2     the K and V cache writes                               -> one copy launch
//   XK_ROPE_APPEND  both of the above (plain RoPE, fp32 cache cells)       -> one launch (rope_append_kernel)
//   XK_GEMM_ADD mul_mat whose only reader is the residual add           -> the GEMV's Add epilogue         (bestla_common.hpp:121-147)
//   XK_GATEUP   mul_mat(w1), silu, mul_mat(w3), mul                     -> ns_hip_fusion_ffn3_gateup      (ip_fusion_ffn.cpp:364-406)
// The intermediate tensors a fused launch does not write (the raw mul_mat results) are checked to have no other reader in the token.
//   carried RMS norms (round 5, ns_norm_link; llama.cpp:178-184, :385-391): rms_norm + mul(gamma) in front of a QKV / gate-up / mul_mat launch
//   whose input tensor came out of a XK_GEMM_ADD launch are not launched at all — that producer also writes fp16(gamma . x) and the tiles'
//   sums of squares, the consumer streams them and divides its dot products by rms(x).  The producer needs the fp16 shadow of ITS input:
//   the attention's merge kernel and the gate/up launch write one when asked (ExecOp::o16).
//   XK_QKV_ROPE (round 6)  XK_QKV with a carried norm + XK_ROPE_APPEND                                 -> ONE launch: the decode GEMV's RoPE epilogue (ns_qkv_rope, as the
//               library's own whole-token path uses it) rotates q and k from a per-token angle table (XK_ROPE_TABLE: one captured launch per token, shared by
//               every layer) and stores k / v into the fp16 mirror AND the reference's fp32 cache cells: 32 launches of a 7B token gone
// A window's PROMPT-sized evaluation (round 6, prefill_pass): the tiled GEMMs multiply fp16 activations, so every producer that can hands its consumer an fp16 copy
// beside the fp32 tensor the graph defines (ExecOp::o16p -> a16p: the attention's output rows, the gate / up product, the normed rows) instead of a conversion pass
// per GEMM, and
//   XK_NORM16      rms_norm + mul(gamma) whose plain result nobody else reads       -> ns_hip_norm_mul_h: gamma . norm(x) as fp32 and fp16, one launch
//   XK_QKV_ROPE_M  XK_QKV + rope(q) + rope(k)                                         -> the fused-QKV GEMM with the RoPE epilogue (as the library's own prefill path):
//                  q, k rotated and v where the graph has them, k / v also as fp16 straight into the kv mirror (no conversion in front of the attention)
enum ExecKind : uint32_t { XK_OP = 0, XK_QKV, XK_ROPE2, XK_DUP2, XK_GEMM_ADD, XK_GATEUP, XK_ROPE_APPEND, XK_QKV_ROPE, XK_ROPE_TABLE, XK_NORM16, XK_QKV_ROPE_M };
constexpr int kXIdx = 10;
struct ExecOp {
  uint32_t xk;
  int idx[kXIdx];    // the plan ops it stands for (-1: unused); XK_OP: idx[0]; a carried norm's rms_norm / mul ride in idx[4], idx[5] of its consumer;
                     // XK_QKV_ROPE: q, k, v mul_mat, rope(q), (norm, mul), rope(k), cpy(k), cpy(v)
  int in_link = -1;  // consumes LinkPlan::links[in_link] (its activations are that link's shadow)
  int out_link = -1; // XK_GEMM_ADD: produces LinkPlan::links[out_link]
  int a16 = -1;      // XK_GEMM_ADD: fp16 shadow of its input = LinkPlan::shadows[a16]
  int o16 = -1;      // attention / XK_GATEUP: also writes the fp16 shadow LinkPlan::shadows[o16] of its output
  int aux = -1;      // XK_ROPE_TABLE: the plan's rope op whose parameters the table is made from (the launch stands for none of the reference's)
  void* a16p = nullptr;  // window, prompt size: fp16 copy of the launch's activations (written by an earlier launch of the window) ...
  void* o16p = nullptr;  // ... and where this launch leaves the fp16 copy of its result
};
// names of the slots of ExecOp::idx that more than one file reads
enum { XI_Q = 0, XI_K = 1, XI_V = 2, XI_ROPE_Q = 3, XI_NORM = 4, XI_NORM_MUL = 5, XI_ROPE_K = 6, XI_DUP_K = 7, XI_DUP_V = 8 };
inline ExecOp xop(uint32_t xk, int a, int b = -1, int c = -1, int d = -1) { return ExecOp{xk, {a, b, c, d, -1, -1, -1, -1, -1, -1}}; }
struct NormLink {
  const float* gamma;
  float eps;
  int n, stride;           // norm size; floats per row of the sums (a multiple of 4 >= ceil(n / 16))
  size_t h_off, s_off;     // fp16(gamma . x) and the tile sums inside the plan's link memory
};
// the device memory a plan's carried norms need, as offsets (ns_route.cpp allocates `bytes`)
struct LinkPlan {
  std::vector<NormLink> links;  // carried norms of the plan
  std::vector<size_t> shadows;  // fp16 shadows
  size_t rope_tab_off = 0;      // the RoPE angle table of XK_QKV_ROPE launches
  size_t bytes = 0;
};
// the launches [xbeg, xend) of a plan stand for the reference's launches [beg, end): a segment is replayed when launch end - 1 has matched
struct SegmentCut {
  int beg, end, xbeg, xend;
};
// a window flushed by a copy: the copy's source is read behind the window's last op (a fusion must not leave out a tensor it reads)
struct ExtraRead {
  const char* p = nullptr;
  size_t bytes = 0;
};

// Every switch and tunable of the route.  env_knobs() (ns_route.cpp) reads the environment once; what can change while the process runs is
// filled in per call.
struct RouteKnobs {
  bool fuse = true;          // NS_ROUTE_FUSE=0: one launch per operator
  bool rope_append = true;   // NS_ROUTE_ROPE_APPEND=0: no XK_ROPE_APPEND
  bool qkv_rope = true;      // NS_ROUTE_QKV_ROPE=0: no XK_QKV_ROPE
  bool prefill_fuse = true;  // NS_ROUTE_PREFILL_FUSE=0: no prefill_pass
  bool links_env = true;     // NS_ROUTE_LINKS=0: no carried norms (ns_hip_route_set_enabled(3 / 5) overrides it)
  // launches per segment; measured on the 7B-shaped model, 355 launches per token: 12 -> 378 tok/s, 24 -> 392, 64 -> 403 —
  // fewer graph launches on the host; the first segment still starts after a few dozen comparisons (NS_ROUTE_SEG)
  int seg = 64;
  // the FIRST segment is shorter: the GPU starts on a token when the reference's executor has handed over its first 16 launches, not its
  // first third (with the norms carried 64 launches are ~210 of the reference's nodes) — NS_ROUTE_SEG0, launches.  Worth little
  // (profiles/r05r_route_carried_norms.txt: 64 / 16 / 6 -> 429 / 436 / 434 tok/s at n_ctx 2048, 451 / 454 / 436 at 512): what precedes a token's
  // first launch is the reference building its graph, not this comparison loop.
  int seg0 = 16;
  bool window = true;     // NS_ROUTE_WINDOW=0 (or NS_DEVICE_REPLAY=0): every op launches when it is handed over
  bool replay = true;     // NS_DEVICE_REPLAY=0: no plans
  bool lazy_sync = true;  // NS_ROUTE_LAZY_SYNC=0: wait where the caller asked
  bool timing = false;    // NS_ROUTE_TIMING
  bool debug = false;     // NS_ROUTE_DEBUG
  int dump = 0;           // NS_ROUTE_DUMP: plan ops printed when a plan is made
  // ---- per call ----
  bool kv16 = true;   // the fp16 kv mirror is on (kv16_enabled())
  bool links = true;  // carried norms are on
};
inline bool links_wanted(const RouteKnobs& kn) { return kn.fuse && kn.links; }  // a plan is first tried with carried norms

// The four questions the planner asks about the device.  The library's answers are today's functions (ns_route.cpp); the test's are a table.
struct RouteEnv {
  virtual ~RouteEnv() = default;
  virtual bool mirror_of_cell(const void* cell, KvMirrorArgs* out) = 0;                        // kvm_args_for_cell
  virtual bool mirror_for_producer(const void* k32, const void* v32, int heads_kv, int hs, int n_ctx, int n_past, int m, _Float16** k16,
                                   _Float16** v16) = 0;                                        // kvm_for_producer
  virtual void* scratch(size_t bytes, int slot) = 0;                                           // stream_scratch on the route's queue
  virtual bool weight_carries_norm(const ns_weight* w) = 0;                                    // route_link_weight_ok
};

// ---- ns_route_fuse.cpp ----
struct TokenPlan {
  std::vector<PlanOp> ops;
  long long act_delta = 0;
  std::unordered_set<const void*> act_ptrs;  // plan addresses of the shifted pointers
};
struct NoPlan {
  const char* why = nullptr;  // nullptr: there is a plan
  long at = -1;               // the op the two traces part at
  bool differs = false;       // ... in a field: worth printing both ops under NS_ROUTE_DEBUG
};
// two consecutive tokens' traces -> the plan (cur's values, what moves per token), or why there is none
NoPlan diff_tokens(const std::vector<RouteOp>& prev, const std::vector<RouteOp>& cur, RouteEnv& env, TokenPlan* out);
// the launches of a plan, fused; with_links: carried norms and the fused QKV + RoPE launch, whose device memory `lp` describes
std::vector<ExecOp> plan_launches(const std::vector<PlanOp>& plan, const RouteKnobs& kn, RouteEnv& env, bool with_links, LinkPlan* lp);
// the launches of a window (ops handed over and not replayed), fused; extra: the source of the copy that ends it
std::vector<ExecOp> window_launches(const std::vector<PlanOp>& w, const RouteKnobs& kn, RouteEnv& env, const ExtraRead& extra);
// segments of about kn.seg launches (the first: kn.seg0); empty: the launches do not cover the plan
std::vector<SegmentCut> cut_segments(const std::vector<ExecOp>& xops, const std::vector<PlanOp>& plan, const RouteKnobs& kn);
// where the cpy node `d` puts element (head, dim) of a packed [heads_kv][head_size] row: cell = dst + head * *sh + dim * *sd floats.  false: not that shape
bool cell_strides(const RouteOp& d, long long hs, long long heads_kv, long long* sd, long long* sh);

// ---- ns_route_exec.cpp ----
// a plan's link memory as a launch sees it (a window has none)
struct LinkMem {
  char* mem = nullptr;
  const LinkPlan* lp = nullptr;
};
// the calling thread is inside a launch the route issues, until the guard ends; nests (the previous state comes back).  The outermost one
// also clears what a launch may have set for its kernels: g_affine, g_kvm
struct ExecGuard {
  ExecGuard();
  ~ExecGuard();
  ExecGuard(const ExecGuard&) = delete;
  ExecGuard& operator=(const ExecGuard&) = delete;

 private:
  bool was_;
};
int execute(const RouteOp& op, hipStream_t st);  // one operator, as the reference asked for it
// one launch of a plan (inside a stream capture; the device counter kdev moves what moves) or of a window (kdev == nullptr: plain values, launched now)
int issue_launch(const ExecOp& xo, const std::vector<PlanOp>& plan, const LinkMem& lm, const int* kdev, hipStream_t st);
int flush_lazy_node();  // the norm / silu node the glue's peephole holds back, launched as one of the route's own

}  // namespace ns
