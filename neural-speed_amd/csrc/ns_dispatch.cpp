// ns_dispatch.cpp — which kernel serves a call: the single forward (forward_impl), the fused QKV, QKV + RoPE, gate/up and FFN entries
// (ns_hip_*forward*, ns_hip_fusion_*) and the device route's two QKV launches.  Every rule the entries share is stated once, in the
// helpers below; what an entry adds to a shared rule (no shuffle, no rejected load, equal widths, the compute mode, gemm3_takes) is
// written at its call site, so that the sites differ visibly where they differ.
//
// Mirrors the reference's operator boundary:
//   neural_speed/core/layers/inner_product.cpp:20-36, ip_fusion_qkv.cpp:155-307, ip_fusion_ffn.cpp:724-779
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ns_api_int.h"

using namespace ns;  // NOLINT

namespace {
// numerics mode (ns_hip_set_compute_mode / NS_COMPUTE): 0 = fp16 activations x dequantised weights, fp32 accumulate
// (default); 1 = the reference's int8-compute semantics for integer weights (ns_i8ref.hip)
int env_compute_mode() {
  const char* e = getenv("NS_COMPUTE");
  return e && (!strcmp(e, "ref_int8") || !strcmp(e, "1")) ? NS_COMPUTE_REF_INT8 : NS_COMPUTE_FP16;
}
std::atomic<int> g_compute_mode{env_compute_mode()};
bool ref_int8_for(const ns_weight* w) { return g_compute_mode.load() == NS_COMPUTE_REF_INT8 && w && i8ref_supported(w); }

// rows up to which the weight-streaming kernel is used; above, the tiled MFMA GEMM (measured crossover)
constexpr int kSmallMMax = 64;
// a carried RMS norm (ns_norm_link) is honoured by gemv_kernel only: refuse everything that would leave its envelope
bool link_ok(const ns_norm_link* link, const ns_weight* w, int m, const void* dA16) {
  if (m > 16 || !dA16 || w->shuf || ref_int8_for(w)) {
    set_error("norm link: needs m <= 16, the fp16 shadow of A, no activation shuffle and the fp16 compute mode");
    return false;
  }
  if (link->in_ssq && (link->in_parts < 1 || link->norm_size < 1 || link->in_stride < link->in_parts || (link->in_stride & 3) ||
                       (reinterpret_cast<uintptr_t>(link->in_ssq) & 15))) {
    set_error("norm link: in_ssq must be 16-byte aligned with in_stride >= in_parts, a multiple of 4");
    return false;
  }
  return true;
}
// the producer side of a norm link (this launch leaves the sums for the next norm) exists on single-matrix forwards only
bool producer_link(const ns_norm_link* link) { return link && (link->out_gamma || link->out_ssq); }
bool refuse_producer_link(const ns_norm_link* link, const char* entry) {  // entry: the error string's prefix, "qkv:" ...
  if (!producer_link(link)) return false;
  set_error(std::string(entry) + " the producer side of a norm link needs a single-matrix forward");
  return true;
}

// `count` weights one fused launch can stream side by side: one K, one quantization format
bool one_format(const ns_weight* const* ws, int count) {
  for (int i = 1; i < count; i++)
    if (ws[i]->k != ws[0]->k || !same_quant(ws[i], ws[0])) return false;
  return true;
}
bool any_shuf(const ns_weight* const* ws, int count) { return std::any_of(ws, ws + count, [](const ns_weight* w) { return w->shuf != nullptr; }); }
bool any_load_failed(const ns_weight* const* ws, int count) { return std::any_of(ws, ws + count, [](const ns_weight* w) { return w->load_failed; }); }
// int8-reference mode: two weights share one activation quantization when K and the group size agree
bool shares_act_quant(const ns_weight* a, const ns_weight* b) {
  return ref_int8_for(a) && ref_int8_for(b) && a->k == b->k && a->blocksize == b->blocksize && !a->shuf && !b->shuf;
}

// ---- launch arguments ----
SmallMArgs base_args(const float* dA, const void* dA16, int lda, int m, int ldc) {
  SmallMArgs a{};
  a.a = dA, a.a16 = dA16, a.lda = lda, a.m = m, a.ldc = ldc;
  return a;
}
SmallMArgs single_args(const float* dA, const void* dA16, int lda, int m, int ldc, const ns_weight* w, float* dC, void* dC16,
                       int epilogue, const float* dD, int ldd) {
  SmallMArgs a = base_args(dA, dA16, lda, m, ldc);
  a.nseg = 1;
  a.seg[0] = {w, dC, dC16};
  a.epilogue = epilogue, a.d = dD, a.ldd = ldd;
  return a;
}
// q, k, v side by side in one launch, each output at its own tensor (the device route's graph) ...
SmallMArgs qkv_args_at(const float* dA, const void* dA16, int lda, int m, int ldc, const ns_weight* const* ws, float* cq, float* ck,
                       float* cv) {
  SmallMArgs a = base_args(dA, dA16, lda, m, ldc);
  a.nseg = 3;
  a.seg[0] = {ws[0], cq, nullptr}, a.seg[1] = {ws[1], ck, nullptr}, a.seg[2] = {ws[2], cv, nullptr};
  a.epilogue = NS_EPI_NONE;
  return a;
}
// ... or one after the other in dC (ip_fusion_qkv.cpp:84-86) and, where the caller has one, in the fp16 shadow dC16 alike.
// cache_only: k / v go to the RoPE epilogue's kv cache alone (no output of their own)
SmallMArgs qkv_args(const float* dA, const void* dA16, int lda, int m, int ldc, const ns_weight* const* ws, float* dC,
                    void* dC16 = nullptr, bool cache_only = false) {
  const size_t step = size_t(m) * ldc;
  SmallMArgs a = qkv_args_at(dA, dA16, lda, m, ldc, ws, dC, cache_only ? nullptr : dC + step, cache_only ? nullptr : dC + 2 * step);
  for (int i = 0; i < 3 && dC16; i++) a.seg[i].c16 = static_cast<uint16_t*>(dC16) + i * step;
  return a;
}
// gate / up pair: act(A W1) * (A W3) -> dTmp2 (+ its fp16 shadow), act(A W1) -> dTmp1 where the caller wants it
SmallMArgs gateup_args(const float* dA, const void* dA16, const ns_weight* w1, const ns_weight* w3, float* dTmp1, float* dTmp2,
                       void* dTmp2_16, int seq, int act) {
  SmallMArgs a = base_args(dA, dA16, w1->k, seq, w1->n);
  a.nseg = 2;
  a.seg[0] = {w1, dTmp2, dTmp2_16};
  a.seg[1] = {w3, dTmp2, nullptr};
  a.epilogue = act;
  a.dual = true;
  a.c2 = dTmp1;
  return a;
}

// rows from which the TILED kernel serves a weight of this shape although most of its tile is padding (measurements: forward_impl)
int tiled_from_rows(const ns_weight* w) {
  return w->ntiles >= 512 ? 17 : w->ntiles >= 256 ? (w->k >= 8192 ? 17 : 33) : 1 << 30;
}

// int8-reference decode launch: the kernel quantizes the activations itself where it can; where it cannot it says so, the quantizer
// launch runs, and the launch is repeated on the codes
hipError_t launch_gemv_i8(const SmallMArgs& a, I8Act* q, hipStream_t st) {
  hipError_t e = launch_gemv(a, st);
  if (e == hipErrorNotReady) {
    e = i8_quantize_finish(q, st);
    if (e == hipSuccess) e = launch_gemv(a, st);
  }
  return e;
}

}  // namespace

namespace ns {
bool same_quant(const ns_weight* a, const ns_weight* b) {
  return a->kind == b->kind && a->blocksize == b->blocksize && a->scale_dt == b->scale_dt && a->asym == b->asym && a->qtype == b->qtype;
}

int forward_impl(const float* dA, const ns_weight* w, float* dC, int m, int lda, int ldc, int epilogue, const float* dD, int ldd,
                 hipStream_t st, const void* dA16, void* dC16, bool reuse_aq, const ns_norm_link* link) {
  if (!w || (!dA && !dA16) || (!dC && !dC16) || m <= 0) {
    set_error("forward: null argument");
    return -1;
  }
  if (w->load_failed) {
    set_error("forward: this weight's load was rejected (ns_hip_weight_finish_load)");
    return -1;
  }
  if (!dA || !dC) {
    // fp16-only activations (the producer wrote its shadow only) and / or an fp16-only output (the consumer is this library's next
    // GEMM): the tiled kernel multiplies fp16 activations as they are and can leave the fp32 store out (round 5)
    if (w->shuf || ref_int8_for(w) || link || !gemm3_takes(w)) {
      set_error("forward: fp16-only activations / outputs need a weight the tiled kernel takes as is (no act-order shuffle, no int8-reference mode; fp8 with the g3_f8 switch on and group scales within its range rule)");
      return -1;
    }
    const hipError_t e = launch_gemm2(single_args(dA, dA16, lda, m, ldc, w, dC, dC16, epilogue, dD, ldd), st);
    if (e == hipErrorNotSupported) {
      set_error("forward: fp16-only activations / outputs are outside the tiled kernel's envelope (K a multiple of 64, lda a multiple of 8, 16-byte aligned)");
      return -1;
    }
    return hip_ok(e, "gemm launch (fp16-only operand)") ? 0 : -1;
  }
  if (link && !link_ok(link, w, m, dA16)) return -1;
  if (!smallm_supported(w, m)) {
    set_error("forward: weight format not supported");
    return -1;
  }
  if (w->shuf) {  // GPTQ act-order blob: gather A'[j] = A[shuf[j]] into scratch first (prologue_a.h:322-330)
    float* ga = static_cast<float*>(stream_scratch(st, size_t(m) * w->k * 4, SLOT_GATHERED_A));
    if (!ga) {
      set_error("forward: no scratch for the activation shuffle (out of device memory)");
      return -1;
    }
    if (!hip_ok(launch_gather_cols(dA, lda, w->shuf, ga, m, w->k, st), "activation shuffle")) return -1;
    dA = ga;
    lda = w->k;
    dA16 = nullptr;  // the caller's fp16 shadow is in the unshuffled order
  }
  if (ref_int8_for(w) && m <= 4) {  // decode-sized: the streaming kernel's int8-reference variant (gemv_kernel XV = 3)
    I8Act q;
    if (hip_ok(i8_quantize_for_decode(dA, lda, w, m, st, reuse_aq && !w->shuf, &q), "activation quantization")) {
      SmallMArgs a = single_args(dA, nullptr, lda, m, ldc, w, dC, dC16, epilogue, dD, ldd);
      a.i8 = &q;
      int rc;
      if (launched(launch_gemv_i8(a, &q, st), "int8-reference decode launch", &rc)) return rc;
      reuse_aq = false;  // outside that kernel's envelope: the general int8-reference kernel, with its own scratch
    } else {
      return -1;
    }
  }
  if (ref_int8_for(w))  // opt-in: quantize A to u8 per k-block and accumulate integer dots, like the CPU int8 cores
    return hip_ok(launch_i8ref(dA, lda, w, dC, dC16, m, ldc, epilogue, dD, ldd, st, reuse_aq && !w->shuf),
                  "int8-reference forward") ? 0 : -1;
  // M <= 64: weight-streaming kernel (HBM-bound); larger M: tiled MFMA GEMM (weights reused across 128 rows)
  SmallMArgs a = single_args(dA, dA16, lda, m, ldc, w, dC, dC16, epilogue, dD, ldd);
  a.link = link;
  static const int small_max = getenv("NS_SMALLM_MAX") ? atoi(getenv("NS_SMALLM_MAX")) : kSmallMMax;  // diagnostics
  // Up to 16 rows the streaming kernel always wins.  From 17 to 64 rows every 16-column workgroup of it stages all rows
  // of A over the whole K from L2, ntiles x m x K x sizeof(A element) bytes in total at about 6 TB/s: measured against
  // the tiled GEMM (scripts/m_small_sweep.py) the break-even is near 140 MB of such staging traffic — 4096 x 4096 stays
  // on the streaming kernel up to 64 rows with an fp16 shadow (21 vs 25 us), 14336 x 4096 leaves it at 17 (53 vs 44 us
  // at 32 rows), fp32 activations leave earlier.
  double staging = double(w->ntiles) * m * w->k * (dA16 ? 2.0 : 4.0);
  // Where the TILED kernel (64-row tile up to 64 rows) beats the streaming one although most of its tile is padding — every
  // 16-column workgroup of the streaming kernel stages all rows of A, the tiled kernel's 128-column workgroups share them
  // (round 3, scripts/m_sweep.py, profiles/r03_m_sweep.txt; us, streaming -> tiled):
  //   32000 x 4096 (lm_head)   8 rows 39.8 -> 32.1, 16 rows 53.4 -> 32.6   (4 rows: 28.9 vs 32.1, stays)
  //   11008 x 4096             16 rows 17.2 -> 16.7, 17 rows 33.0 -> 17.5, 64 rows 44.8 -> 20.8
  //   4096 x 11008             16 rows 24.1 -> 19.7 (12 rows level),  4096 x 4096: 33 rows 15.8 -> 13.4 (below: level or behind)
  // fp8 weights keep the old rule up to 64 rows (streaming / first-generation kernels) and take the tiled kernel from 65 (launch_gemm2
  // refuses them below, docs/kernels/gemm3.md).  NS_TILED_MIN_M: diagnostics (A-B runs).
  static const int tiled_env = getenv("NS_TILED_MIN_M") ? atoi(getenv("NS_TILED_MIN_M")) : 0;
  // Up to 16 rows every call stays on the streaming kernels all the same: their accumulation is exact in fp32 (3e-5 from the
  // fp64 product of the fp16-rounded activations, tests/test_gpu_fullsize.py), the tiled kernel rounds scaled weights to fp16
  // (2e-4), and a decode step's numerics should not depend on the shape of the matrix.
  const int tiled_from = tiled_env > 0 ? tiled_env : tiled_from_rows(w);
  const bool wide_tiled = m >= tiled_from && (w->kind != WK_F8 || (m > 64 && gemm3_takes(w))) && !getenv("NS_SMALLM_MAX");
  const bool small = !wide_tiled && (m <= 16 || (m <= small_max && (staging <= 140e6 || getenv("NS_SMALLM_MAX") != nullptr)));
  // fp32 activations, several rows, many column tiles: one conversion pass to fp16 (about 2 us) halves what every
  // workgroup of the streaming kernel stages (14336 x 4096 at 16 rows: 39 -> 24 us; at 8 rows: 25 -> 18 us)
  if (small && !dA16 && m >= 6 && staging > 60e6 && lda == w->k && w->k % 8 == 0) {
    void* sc = stream_scratch(st, size_t(m) * w->k * 2, SLOT_A16);
    if (sc && hip_ok(launch_cvt_a16(dA, sc, m, w->k, lda, w->k, st), "activation fp16 pass")) a.a16 = sc;
  }
  if (!hip_ok(small ? launch_smallm(a, st) : launch_gemm(a, st), "gemm launch")) return -1;
  return 0;
}

// the device route's replayed QKV launch (ns_route.cpp XK_QKV_ROPE): one row, carried norm on the input, RoPE + fp16 mirror + fp32 cache cells in the epilogue
int qkv_rope_route_forward(const float* dA, const void* dA16, const ns_weight* wq, const ns_weight* wk, const ns_weight* wv, float* cq, float* ck,
                           float* cv, int lda, const ns_norm_link* link, const ns_qkv_rope* rope, const QkvRopeRoute* rr, hipStream_t st) {
  if (!have_device()) return -1;
  const ns_weight* ws[3] = {wq, wk, wv};
  if (!rr) {  // a window's prompt-sized launch (rows: rope->flags' place is taken by the caller's m in `lda`'s partner below): the tiled GEMM carries the epilogue
    set_error("route qkv+rope: prompt-sized calls go through qkv_rope_route_forward_m");
    return -1;
  }
  if (rope && ((rope->flags & NS_QKV_ROPE_NEOX) || rope->mode != 0)) {
    set_error("route qkv+rope: the replayed route is llama's, RoPE mode 0");
    return -1;
  }
  if (!wq || !wk || !wv || !dA16 || !cq || !ck || !cv || !rope) {
    set_error("route qkv+rope: null argument");
    return -1;
  }
  const bool same = !ref_int8_for(wq) && one_format(ws, 3) && !any_shuf(ws, 3) && !any_load_failed(ws, 3);
  if (!same || !smallm_supported(wq, 1) || producer_link(link) || (link && !link_ok(link, wq, 1, dA16))) {
    if (same) set_error("route qkv+rope: the launch cannot carry this norm / these weights");
    else set_error("route qkv+rope: needs three weights of one format in the fp16 compute mode");
    return -1;
  }
  SmallMArgs a = qkv_args_at(dA, dA16, lda, 1, wq->n, ws, cq, ck, cv);
  a.link = link;
  a.rope = rope;
  a.rope_route = rr;
  return hip_ok(launch_smallm(a, st), "route qkv+rope launch") ? 0 : -1;
}
// ... and of a window's prompt-sized evaluation (m > 16): the tiled GEMM's fused-QKV launch rotates q / k from a table of m positions, writes the three fp32
// tensors where the graph has them and k / v as fp16 into the kv mirror (rope->kcache16 / vcache16).  -2: the launch does not take this shape (the caller keeps
// its separate launches)
int qkv_rope_route_forward_m(const float* dA, const void* dA16, const ns_weight* wq, const ns_weight* wk, const ns_weight* wv, float* cq, float* ck, float* cv, int m,
                             int lda, int ldc, const ns_qkv_rope* rope, hipStream_t st) {
  if (!have_device()) return -1;
  const ns_weight* ws[3] = {wq, wk, wv};
  if (!wq || !wk || !wv || !dA || !cq || !ck || !cv || !rope || m <= 16) return -2;
  // (fp8 weights from 65 rows: the separate launches the caller keeps below that are the ones that served such a window before)
  const bool one = !ref_int8_for(wq) && (wq->kind != WK_F8 || (m > 64 && gemm3_takes(wq) && gemm3_takes(wk) && gemm3_takes(wv))) &&
                   one_format(ws, 3) && !any_shuf(ws, 3) && !any_load_failed(ws, 3);
  if (!one) return -2;
  SmallMArgs a = qkv_args_at(dA, dA16, lda, m, ldc, ws, cq, ck, cv);
  a.rope = rope;
  const hipError_t e = launch_gemm2(a, st);
  if (e == hipErrorNotSupported) return -2;
  return hip_ok(e, "route qkv+rope GEMM launch") ? 0 : -1;
}
bool route_link_weight_ok(const ns_weight* w) { return w && !w->shuf && !w->load_failed && !ref_int8_for(w) && w->kind != WK_F8 && smallm_supported(w, 1); }
}  // namespace ns

extern "C" {

int ns_hip_set_compute_mode(int mode) {
  if (mode != NS_COMPUTE_FP16 && mode != NS_COMPUTE_REF_INT8) {
    set_error("compute mode: 0 (fp16 activations) or 1 (reference int8 compute)");
    return -1;
  }
  return g_compute_mode.exchange(mode);
}
int ns_hip_get_compute_mode(void) { return g_compute_mode.load(); }

int ns_hip_f32f32_forward(const float* dA, const ns_weight* w, float* dC, int m, int lda, int ldc, int epilogue,
                          const float* dD, int ldd, void* stream) {
  if (!have_device()) return -1;
  return forward_impl(dA, w, dC, m, lda, ldc, epilogue, dD, ldd, (hipStream_t)stream);
}

int ns_hip_fusion_qkv_forward(const float* dA, const ns_weight* wq, const ns_weight* wk, const ns_weight* wv, float* dC,
                              int m, int lda, int ldc, void* stream) {
  return ns_hip_fusion_qkv_forward_h(dA, nullptr, wq, wk, wv, dC, nullptr, m, lda, ldc, stream);
}

int ns_hip_f32f32_forward_h(const float* dA, const void* dA16, const ns_weight* w, float* dC, void* dC16, int m, int lda,
                            int ldc, int epilogue, const float* dD, int ldd, void* stream) {
  return ns_hip_f32f32_forward_x(dA, dA16, w, dC, dC16, m, lda, ldc, epilogue, dD, ldd, nullptr, stream);
}

int ns_hip_f32f32_forward_x(const float* dA, const void* dA16, const ns_weight* w, float* dC, void* dC16, int m, int lda,
                            int ldc, int epilogue, const float* dD, int ldd, const ns_norm_link* link, void* stream) {
  if (!have_device()) return -1;
  return forward_impl(dA, w, dC, m, lda, ldc, epilogue, dD, ldd, (hipStream_t)stream, dA16, dC16, false, link);
}

int ns_hip_fusion_qkv_forward_h(const float* dA, const void* dA16, const ns_weight* wq, const ns_weight* wk,
                                const ns_weight* wv, float* dC, void* dC16, int m, int lda, int ldc, void* stream) {
  return ns_hip_fusion_qkv_forward_x(dA, dA16, wq, wk, wv, dC, dC16, m, lda, ldc, nullptr, stream);
}

int ns_hip_fusion_qkv_rope_forward_x(const float* dA, const void* dA16, const ns_weight* wq, const ns_weight* wk,
                                     const ns_weight* wv, float* dC, int m, int lda, int ldc, const ns_norm_link* link,
                                     const ns_qkv_rope* rope, void* stream) {
  if (!have_device()) return -1;
  if (!wq || !wk || !wv || (!dA && !(dA16 && m > 16)) || !dC || !rope || m < 1) {  // (dA may be NULL at prefill size: fp16-only activations)
    set_error("qkv+rope: null argument");
    return -1;
  }
  if (refuse_producer_link(link, "qkv+rope:")) return -1;
  if (rope->flags & ~(NS_QKV_ROPE_KV_CACHE_ONLY | NS_QKV_ROPE_NEOX)) {  // (`flags` is the struct's newest field — a caller built against the older header passes what lay behind it)
    set_error("qkv+rope: unknown bits in ns_qkv_rope::flags (zero the struct before filling it: the field was added in round 5)");
    return -1;
  }
  const bool neox = (rope->flags & NS_QKV_ROPE_NEOX) != 0;
  if (neox != (rope->mode == 2)) {
    // mode 2 without the flag: the unchanged contract (callers keep ns_hip_fusion_qkv_forward_x + ns_hip_rope_qkv_append); the flag says the table is mode 2's
    set_error(neox ? "qkv+rope: NS_QKV_ROPE_NEOX goes with mode 2 only"
                   : "qkv+rope: mode 2 (NeoX) needs NS_QKV_ROPE_NEOX in flags and the table of ns_hip_rope_cos_sin_mode(mode 2); other modes than 0 / 2 have no epilogue");
    return -1;
  }
  if (neox) {
    if (rope->n_dims != rope->head_size || rope->head_size < 32) {
      set_error("qkv+rope (NeoX): whole-head rotation only (n_dims == head_size)");
      return -1;
    }
    if (m <= 16 ? (rope->head_size % 32) != 0 : (rope->head_size != 32 && rope->head_size != 64 && rope->head_size != 128)) {
      set_error(m <= 16 ? "qkv+rope (NeoX) at decode size: head_size must be a multiple of 32 (a workgroup streams both 16-column tiles of a pair)"
                        : "qkv+rope (NeoX) at prefill size: head_size 32, 64 or 128 (a head inside one 128-column block); use ns_hip_fusion_qkv_forward_h + ns_hip_rope_qkv_append for this head size");
      return -1;
    }
  }
  const ns_weight* ws[3] = {wq, wk, wv};
  if (m > 16) {  // prefill size (round 5): the tiled GEMM's fused-QKV launch carries the epilogue; k / v optionally to the cache only
    const bool one = !ref_int8_for(wq) && !link && gemm3_takes(wq) && gemm3_takes(wk) && gemm3_takes(wv) && one_format(ws, 3) &&
                     !any_shuf(ws, 3) && !any_load_failed(ws, 3);
    if (one) {
      SmallMArgs a = qkv_args(dA, dA16, lda, m, ldc, ws, dC, nullptr, (rope->flags & NS_QKV_ROPE_KV_CACHE_ONLY) != 0);
      a.rope = rope;
      int rc;
      if (launched(launch_gemm2(a, (hipStream_t)stream), "qkv+rope GEMM launch", &rc)) return rc;
    }
    if (getenv("NS_ROPE_GEMM_DEBUG")) fprintf(stderr, "qkv+rope at prefill size refused: one format %d, m %d, k %d, n %d %d %d, head_size %d, ldc %d\n", int(one), m, wq->k, wq->n, wk->n, wv->n, rope->head_size, ldc);
    set_error("qkv+rope at prefill size: needs three weights of one format the tiled kernel takes (integer, f4, or fp8 with the g3_f8 switch on), plain whole-head RoPE, head_size a multiple of 4, matrix widths multiples of 128, 16-byte aligned outputs and no norm link");
    return -1;
  }
  const bool same = !ref_int8_for(wq) && m <= 16 && dA16 && one_format(ws, 3) && !any_shuf(ws, 3);
  if (!same || !smallm_supported(wq, m)) {
    set_error("qkv+rope: needs three weights of one format, m <= 16, the fp16 shadow of A and the fp16 compute mode");
    return -1;
  }
  SmallMArgs a = qkv_args(dA, dA16, lda, m, ldc, ws, dC);
  a.link = link;
  a.rope = rope;
  return hip_ok(launch_smallm(a, (hipStream_t)stream), "qkv+rope launch") ? 0 : -1;
}

int ns_hip_fusion_qkv_forward_x(const float* dA, const void* dA16, const ns_weight* wq, const ns_weight* wk,
                                const ns_weight* wv, float* dC, void* dC16, int m, int lda, int ldc,
                                const ns_norm_link* link, void* stream) {
  if (!have_device()) return -1;
  if (!wq || !wk || !wv) {
    set_error("qkv: null weight");
    return -1;
  }
  const ns_weight* ws[3] = {wq, wk, wv};
  bool same = one_format(ws, 3);
  same &= !any_shuf(ws, 3);      // each shuffled weight gathers its own A' (unfused path)
  same &= !ref_int8_for(wq);     // int8-reference mode: three plain forwards share nothing but A
  hipStream_t st = (hipStream_t)stream;
  if (refuse_producer_link(link, "qkv:")) return -1;
  if (link && !link_ok(link, wq, m, dA16)) return -1;
  int rc;
  if (ref_int8_for(wq) && m <= 4 && !link) {  // int8-reference numerics, decode-sized: ONE activation quantization + one launch
    const bool same8 = ref_int8_for(wk) && ref_int8_for(wv) && one_format(ws, 3) && !any_shuf(ws, 3);
    I8Act q;
    if (same8 && i8_quantize_for_decode(dA, lda, wq, m, st, false, &q) == hipSuccess) {
      SmallMArgs a = qkv_args(dA, nullptr, lda, m, ldc, ws, dC, dC16);
      a.i8 = &q;
      if (launched(launch_gemv_i8(a, &q, st), "int8-reference qkv launch", &rc)) return rc;
    }
  }
  // GEMM size: the three matrices side by side in ONE launch of the tiled kernel
  if (same && m > 64 && !link && launched(launch_gemm2(qkv_args(dA, dA16, lda, m, ldc, ws, dC, dC16), st), "qkv GEMM launch", &rc))
    return rc;
  if (!same || m > 64) {  // fall back to three launches (still on the GPU)
    for (int i = 0; i < 3; i++)
      if (forward_impl(dA, ws[i], dC + size_t(i) * m * ldc, m, lda, ldc, NS_EPI_NONE, nullptr, 0, st, dA16,
                       dC16 ? static_cast<uint16_t*>(dC16) + size_t(i) * m * ldc : nullptr, i > 0 && shares_act_quant(ws[i], ws[0]), link))
        return -1;
    return 0;
  }
  SmallMArgs a = qkv_args(dA, dA16, lda, m, ldc, ws, dC, dC16);
  a.link = link;
  return hip_ok(launch_smallm(a, st), "qkv launch") ? 0 : -1;
}

int ns_hip_fusion_ffn3_gateup(const float* dA, const ns_weight* w1, const ns_weight* w3, float* dTmp1, float* dTmp2,
                              int seq, int act, void* stream) {
  return ns_hip_fusion_ffn3_gateup_h(dA, nullptr, w1, w3, dTmp1, dTmp2, nullptr, seq, act, stream);
}

int ns_hip_fusion_ffn3_gateup_h(const float* dA, const void* dA16, const ns_weight* w1, const ns_weight* w3,
                                float* dTmp1, float* dTmp2, void* dTmp2_16, int seq, int act, void* stream) {
  return ns_hip_fusion_ffn3_gateup_x(dA, dA16, w1, w3, dTmp1, dTmp2, dTmp2_16, seq, act, nullptr, stream);
}

int ns_hip_fusion_ffn3_gateup_x(const float* dA, const void* dA16, const ns_weight* w1, const ns_weight* w3,
                                float* dTmp1, float* dTmp2, void* dTmp2_16, int seq, int act, const ns_norm_link* link,
                                void* stream) {
  if (!have_device()) return -1;
  if (!w1 || !w3 || (!dTmp2 && !dTmp2_16) || (!dA && !dA16)) {  // (dA may be NULL at GEMM size: fp16-only activations, as for the single forward)
    set_error("ffn3 gate/up: null argument");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int fin = w1->k, fmid = w1->n;
  const ns_weight* ws[2] = {w1, w3};
  const bool same = one_format(ws, 2) && w3->n == fmid && !any_shuf(ws, 2);
  const bool ref8 = ref_int8_for(w1);  // int8-reference mode: the two GEMVs and the activation stay separate operators
  int rc;
  // GEMM size (round 5): ONE launch of the tiled kernel on gate / up tile pairs — act(A W1) * (A W3) is formed in registers, so
  // neither tmp1 nor an fp32 tmp2 has to exist (each is written only if the caller hands a pointer: the reference's graph treats
  // both as scratch, ne_layers.c:2573-2576); before, W1 wrote tmp1 (fp32), W3 read it back and wrote tmp2 (fp32 + fp16)
  // (fp8 weights: from 65 rows; from 17 like the rest only where nothing else serves the call — fp16-only activations)
  const bool f8_rows = w1->kind != WK_F8 || (gemm3_takes(w1) && gemm3_takes(w3) && (seq > 64 || !dA));
  if (same && !ref8 && !link && seq > 16 && (seq > 64 || seq >= tiled_from_rows(w1)) && f8_rows && (dTmp2 || dTmp2_16) &&
      smallm_supported(w1, seq) &&
      launched(launch_gemm2(gateup_args(dA, dA16, w1, w3, dTmp1, dTmp2, dTmp2_16, seq, act), st), "ffn gate/up GEMM launch", &rc))
    return rc;
  if (!dA) {
    set_error("ffn3 gate/up: fp16-only activations need the tiled kernel's fused launch (matching formats, more than 16 rows, K a multiple of 64, 16-byte aligned)");
    return -1;
  }
  if (!dTmp2) {  // the paths below produce the fp32 product
    dTmp2 = static_cast<float*>(stream_scratch(st, size_t(seq) * fmid * 4, SLOT_FFN_TMP2));
    if (!dTmp2) {
      set_error("ffn3 gate/up: no scratch for tmp2 (out of device memory)");
      return -1;
    }
  }
  if (same && smallm_dual_ok(seq) && smallm_supported(w1, seq) && !ref8) {
    if (refuse_producer_link(link, "ffn gate/up:") || (link && !link_ok(link, w1, seq, dA16))) return -1;
    SmallMArgs a = gateup_args(dA, dA16, w1, w3, dTmp1, dTmp2, dTmp2_16, seq, act);
    a.link = link;
    return hip_ok(launch_smallm(a, st), "ffn gate/up launch") ? 0 : -1;
  }
  if (link) {
    set_error("ffn gate/up: a norm link needs the fused launch (matching formats, seq <= 16)");
    return -1;
  }
  if (ref8 && same && seq <= 4 && ref_int8_for(w3)) {  // int8-reference numerics, decode-sized: one quantization, one launch
    I8Act q;
    if (i8_quantize_for_decode(dA, fin, w1, seq, st, false, &q) == hipSuccess) {
      SmallMArgs a = gateup_args(dA, nullptr, w1, w3, dTmp1, dTmp2, dTmp2_16, seq, act);
      a.i8 = &q;
      if (launched(launch_gemv_i8(a, &q, st), "int8-reference gate/up launch", &rc)) return rc;
    }
  }
  if (!dTmp1) dTmp1 = static_cast<float*>(stream_scratch(st, size_t(seq) * fmid * 4, SLOT_FFN_TMP1));
  if (!dTmp1) {
    set_error("ffn3: no scratch for tmp1 on the unfused path (out of device memory)");
    return -1;
  }
  if (forward_impl(dA, w1, dTmp1, seq, fin, fmid, act, nullptr, 0, st, dA16, nullptr)) return -1;
  return forward_impl(dA, w3, dTmp2, seq, fin, fmid, NS_EPI_MUL, dTmp1, fmid, st, dA16, dTmp2_16, shares_act_quant(w3, w1));
}

int ns_hip_fusion_ffn3_forward(const float* dA, const ns_weight* w1, const ns_weight* w2, const ns_weight* w3,
                               float* dTmp1, float* dTmp2, float* dOut, int seq, int act, void* stream) {
  if (!have_device()) return -1;
  return ns_hip_fusion_ffn3_forward_h(dA, nullptr, w1, w2, w3, dTmp1, dTmp2, nullptr, dOut, nullptr, seq, act, stream);
}

int ns_hip_fusion_ffn3_forward_h(const float* dA, const void* dA16, const ns_weight* w1, const ns_weight* w2,
                                 const ns_weight* w3, float* dTmp1, float* dTmp2, void* dTmp2_16, float* dOut,
                                 void* dOut16, int seq, int act, void* stream) {
  if (!have_device()) return -1;
  if (!w1 || !w2 || !w3 || w2->k != w1->n) {
    set_error("ffn3: bad argument");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int fmid = w1->n;
  // GEMM size, no fp32 tmp2 asked for: the intermediate exists as fp16 only (the down projection multiplies fp16 activations anyway);
  // it lives in the caller's dTmp2_16 or in per-stream scratch
  if (!dTmp2 && seq > 16 && !w2->shuf && !ref_int8_for(w2) && (w2->kind != WK_F8 || (gemm3_takes(w2) && (seq > 64 || !dA))) && fmid % 64 == 0) {
    void* t16 = dTmp2_16 ? dTmp2_16 : stream_scratch(st, size_t(seq) * fmid * 2, SLOT_FFN_TMP2_16);
    int rc;
    if (t16 && ns_hip_fusion_ffn3_gateup_h(dA, dA16, w1, w3, dTmp1, nullptr, t16, seq, act, stream) == 0 &&
        launched(launch_gemm2(single_args(nullptr, t16, fmid, seq, w2->n, w2, dOut, dOut16, NS_EPI_NONE, nullptr, 0), st),
                 "ffn down GEMM launch", &rc))
      return rc;
    // (outside the tiled kernel's envelope: the general path below, on an fp32 intermediate)
  }
  if (!dTmp2) dTmp2 = static_cast<float*>(stream_scratch(st, size_t(seq) * fmid * 4, SLOT_FFN_TMP2));
  if (!dTmp2) {
    set_error("ffn3: no scratch for tmp2 (out of device memory)");
    return -1;
  }
  if (ns_hip_fusion_ffn3_gateup_h(dA, dA16, w1, w3, dTmp1, dTmp2, dTmp2_16, seq, act, stream)) return -1;
  return forward_impl(dTmp2, w2, dOut, seq, w1->n, w2->n, NS_EPI_NONE, nullptr, 0, st, dTmp2_16, dOut16);
}

int ns_hip_fusion_ffn2_forward(const float* dA, const ns_weight* w1, const ns_weight* w2, const float* dB1,
                               const float* dB2, float* dTmp1, float* dOut, int seq, bool broadcast_bias, void* stream) {
  if (!have_device()) return -1;
  if (!w1 || !w2 || !dTmp1) {
    set_error("ffn2: null argument");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int fin = w1->k, fmid = w1->n, fout = w2->n;
  if (forward_impl(dA, w1, dTmp1, seq, fin, fmid, dB1 ? NS_EPI_ADD_GELU : NS_EPI_GELU, dB1, broadcast_bias ? 0 : fmid, st))
    return -1;
  return forward_impl(dTmp1, w2, dOut, seq, fmid, fout, dB2 ? NS_EPI_ADD : NS_EPI_NONE, dB2, broadcast_bias ? 0 : fout, st);
}

}  // extern "C"
