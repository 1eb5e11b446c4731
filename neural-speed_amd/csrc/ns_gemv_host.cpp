// ns_gemv_host.cpp — host side of the decode kernel (gemv_kernel, ns_gemv.hip): launch_gemv turns a SmallMArgs into the kernel's
// GemvParams — envelope checks, wave count, LDS layout — and hands it to the launcher of the weight's slice (ns_gemv.h: one
// translation unit of instantiations per weight kind and scales-per-record count); the kernel's tuning state; touch_gemv_module.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdlib>
#include <cstring>

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

// waves per workgroup of a decode launch (one 16-column tile per workgroup, k-steps dealt round-robin to the waves).
// Shared with smallm_kernel so that both kernels split K the same way — bit-identical sums between a caller that passes
// the fp16 shadow of A and an fp32-only caller — wherever this rule alone decides: launch_gemv additionally halves the
// wave count until activations + rings fit in LDS (several rows of a large K), where smallm_kernel keeps the rule's value;
// the two then differ in fp32 summation order only (fp32-only callers of decode shapes are served by gemv_kernel itself
// since round 3, bit-equal to the shadow path: tests/test_gpu_fullsize.py).
static std::atomic<int> g_decode_waves{0};  // ns_hip_set_tuning("gv_nw", n)
void set_decode_waves(int nw) { g_decode_waves.store(nw); }
int decode_waves(int grid, int ks, bool dual) {
  // measured on the 7B shapes (profiles/r02g_sweep.txt): 256 tiles x 32 k-steps (attention output) 16 waves, 256 tiles
  // x 86 k-steps (FFN down) 8 waves (7.5 vs 8.0 us at 16), 768 tiles 4 waves, 2000 tiles (lm_head) 2 waves
  int nw = (grid <= 320 && ks >= 32 && ks <= 48 && !dual) ? 16 : 8;
  if (dual) {
    nw = grid * 4 >= 1300 ? 4 : 8;
  } else {
    const int target_waves = 2560;
    while (nw > 2 && grid * (nw / 2) >= target_waves) nw /= 2;
  }
  static const int env_nw0 = getenv("NS_GV_NW") ? atoi(getenv("NS_GV_NW")) : 0;  // diagnostics
  const int forced = g_decode_waves.load();
  const int env_nw = forced ? forced : env_nw0;
  if (env_nw == 2 || env_nw == 4 || env_nw == 8 || (env_nw == 16 && !dual)) nw = env_nw;
  while (nw > 1 && nw > ks) nw /= 2;
  return nw;
}

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

// hipErrorNotSupported: outside the kernel's envelope — the caller falls back to smallm_kernel
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

hipError_t launch_gemv(const SmallMArgs& a, hipStream_t st) {
  if (gemv_mode() == 0 || a.m < 1 || a.m > kGvMaxRows) return hipErrorNotSupported;
  const int nmat = a.nseg;  // matrices the launch touches (dual: 2)
  // bit-plane formats: every matrix of the launch has its native clone (same shapes and scales, shorter code records) -> stream those
  const bool neox = a.rope && (a.rope->flags & NS_QKV_ROPE_NEOX) != 0;  // the pair mode (GV_MSEGP) streams the widened records
  bool planes = gemv_planes() && !a.i8 && !a.moe && !neox;
  for (int i = 0; i < nmat; i++)
    planes = planes && a.seg[i].w->native && a.seg[i].w->native->scale_dt != DT_F16 && a.seg[i].w->native->pl_bits == a.seg[0].w->native->pl_bits;
  auto pick = [&](const ns_weight* w) { return planes ? static_cast<const ns_weight*>(w->native) : w; };
  const ns_weight* w0 = pick(a.seg[0].w);
  GemvParams p;
  memset(&p, 0, sizeof(p));
  uint32_t tiles = 0;
  uint32_t tbeg[3] = {0, 0xffffffffu, 0xffffffffu};  // absent matrices begin beyond every tile
  const uint8_t* wb[3] = {nullptr, nullptr, nullptr};
  uint32_t soff[3] = {0, 0, 0}, zoff[3] = {0, 0, 0};
  for (int i = 0; i < nmat; i++) {
    const ns_weight* w = pick(a.seg[i].w);
    if (!w->single_span || w->alloc_bytes >= (size_t(1) << 31)) return hipErrorNotSupported;
    wb[i] = reinterpret_cast<const uint8_t*>(w->codes);
    soff[i] = uint32_t(reinterpret_cast<const uint8_t*>(w->scales) - wb[i]);
    zoff[i] = w->zps ? uint32_t(reinterpret_cast<const uint8_t*>(w->zps) - wb[i]) : 0u;
    tbeg[i] = a.dual ? 0u : tiles;
    if (!a.dual || i == 0) tiles += uint32_t(w->ntiles);
    p.mat[i] = GemvMat{wb[i], soff[i], zoff[i], tbeg[i], w->n, a.seg[i].c, static_cast<_Float16*>(a.seg[i].c16)};
  }
  const bool mseg = !a.dual && nmat > 1;
  const int mode = a.dual ? GV_DUAL : (mseg ? (neox ? GV_MSEGP : GV_MSEG) : GV_PLAIN);
  if (neox) {  // whole pairs of tiles per head and matrix: a workgroup per pair
    const int hs = a.rope->head_size;
    if (!mseg || nmat != 3 || a.rope_route || hs < 32 || (hs % 32) != 0) return hipErrorInvalidValue;
    for (int i = 0; i < nmat; i++)
      if (p.mat[i].n % hs != 0 || uint32_t(p.mat[i].n) != 16u * uint32_t(pick(a.seg[i].w)->ntiles)) return hipErrorInvalidValue;
    p.pair_tiles = uint32_t(hs / 32);
    tbeg[1] /= 2, tbeg[2] /= 2;  // in workgroups (p.mat[].tile_begin is not read by the kernel)
  }
  p.wbase0 = wb[0];
  p.wbase1 = wb[1];
  p.s_off0 = soff[0], p.s_off1 = soff[1], p.z_off0 = zoff[0], p.z_off1 = zoff[1];
  p.tb1 = mseg ? tbeg[1] : 0xffffffffu;
  p.tb2 = (mseg && nmat > 2) ? tbeg[2] : 0xffffffffu;
  const uint32_t ks = uint32_t(w0->ksteps);
  const int kstep = w0->kstep_len;
  if (tiles == 0 || ks == 0) return hipErrorNotSupported;

  // staged activations: [rows][ks * KSTEP + 8] halves (int8-reference numerics: [rows][ks * KSTEP + 16] bytes)
  const int rows = a.m;
  const bool i8s = a.i8 != nullptr;
  bool i8q = false;
  const uint32_t row_stride = i8s ? (ks * uint32_t(kstep) + 16) / 2 : ks * uint32_t(kstep) + 8;
  const size_t a_bytes = size_t(rows) * row_stride * 2;
  if (a_bytes > kGvMaxALds) return hipErrorNotSupported;
  uint32_t i8_shift = 0;
  if (i8s) {
    const I8Act& q = *a.i8;
    const bool int_w = w0->kind == WK_INT4 || w0->kind == WK_INT8;
    // a 32-deep slice must lie inside one k-block and inside or outside K; block index by shift (one block: any shift >= 31)
    const bool one_block = q.nblk == 1;
    while (!one_block && (1u << i8_shift) < uint32_t(q.blocksize)) i8_shift++;
    if (!int_w || rows > 4 || a.link || a.rope || (w0->k & 31) || !q.aq || !q.corr || (reinterpret_cast<uintptr_t>(q.aq) & 15) ||
        (reinterpret_cast<uintptr_t>(q.corr) & 15) || (q.ldq & 15) || q.ldq < w0->k ||
        (!one_block && ((1u << i8_shift) != uint32_t(q.blocksize) || q.blocksize < 32)))
      return hipErrorNotSupported;
    if (one_block) i8_shift = 31;
    // XV = 5: quantize inside the launch when the rows are at hand as fp32 and the k-block is 32 .. 256 columns dividing K
    static const bool i8q_off = getenv("NS_I8_INKERNEL") && atoi(getenv("NS_I8_INKERNEL")) == 0;  // A-B runs
    i8q = !i8q_off && q.a32 && !one_block && i8_shift >= 5 && i8_shift <= 8 && w0->k % q.blocksize == 0 && (q.lda32 & 3) == 0 &&
          (w0->k & 3) == 0 && (reinterpret_cast<uintptr_t>(q.a32) & 15) == 0;
    if (!i8q && !q.quantized) return hipErrorNotReady;  // the caller runs the quantizer launch (i8_quantize_finish) and comes back
    p.i8_corr = q.corr;
    p.i8_nblk = uint32_t(q.nblk);
    p.i8_span = (uint32_t(rows) * uint32_t(q.nblk) * 5u + 3u) & ~3u;  // whole words: a buffer load drops a word that straddles the bound (the scratch has the slack)
    p.i8_bshift = i8_shift;
  }
  // fp16 activations with 16-byte aligned rows; several rows need K to fill whole k-steps (a row's padding columns
  // would otherwise read the next row through the descriptor)
  const bool a16 = (i8s && !i8q) || (!i8s && a.a16 != nullptr && (a.lda & 7) == 0 && (w0->k & 7) == 0 && (reinterpret_cast<uintptr_t>(a.a16) & 15) == 0);
  // fp32-only callers: converted while staging (XV = 2); not together with a carried norm / fused RoPE, whose producers
  // always leave a shadow
  const bool moe = a.moe != nullptr;
  if (moe && (a.m != 1 || nmat != (a.dual ? 2 : 1) || a.link || a.rope || i8s || a.a16 || !a.moe->table || !a.moe->id)) return hipErrorNotSupported;
  if (moe) {  // its (row, selection) pairs along grid.y; fused gate / up: the second table, the kernel's one set of strides for both matrices
    const MoeRoute& r = *a.moe;
    if (r.pairs < 1 || r.pairs > 65535 || r.nsel < 1 || int64_t(r.pairs) * r.nsel >= 65536 || (r.a_stride & 3) || r.a_stride < 0 || r.c_stride < 0 ||
        r.d_stride < 0 || std::max({r.a_stride, r.c_stride, r.d_stride}) >= (1ll << 32))
      return hipErrorNotSupported;
    if (a.dual) {
      const ns_weight* w1 = a.seg[1].w;
      if (!r.table1 || a.c2 || w1->n != w0->n || w1->k != w0->k || w1->kind != w0->kind || w1->qtype != w0->qtype || w1->blocksize != w0->blocksize ||
          w1->scale_dt != w0->scale_dt || w1->asym != w0->asym || w1->qstride != w0->qstride || w1->sstride != w0->sstride ||
          w1->zstride != w0->zstride || w1->sps != w0->sps || w1->ksteps != w0->ksteps || w1->srows != w0->srows)
        return hipErrorNotSupported;
    }
  }
  const bool a32 = i8q || (!i8s && !a16 && a.a != nullptr && !a.link && !a.rope && (a.lda & 3) == 0 && (w0->k & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.a) & 15) == 0);
  if (moe && !a32) return hipErrorNotSupported;
  if ((!a16 && !a32) || (rows > 1 && w0->k % kstep != 0)) return hipErrorNotSupported;
  p.a = i8q ? static_cast<const void*>(a.i8->a32) : i8s ? static_cast<const void*>(a.i8->aq) : (a16 ? a.a16 : static_cast<const void*>(a.a));
  // carried RMS norm (ns_norm_link): consumer side stages in_parts floats per row behind A
  size_t ssq_bytes = 0;
  if (i8s) ssq_bytes = (size_t(p.i8_span) + 1023) >> 10 << 10;  // the scales / zero points span sits where a carried norm's sums would
  if (a.link) {
    const ns_norm_link& k = *a.link;
    if (k.in_ssq) {
      if (k.in_parts < 1 || k.in_stride < k.in_parts || (k.in_stride & 3) || (reinterpret_cast<uintptr_t>(k.in_ssq) & 15) ||
          k.norm_size < 1)
        return hipErrorInvalidValue;
      ssq_bytes = size_t(rows) * ((size_t(k.in_parts) * 4 + 1023) >> 10 << 10);
      if (ssq_bytes > 32 * 1024) return hipErrorNotSupported;  // at most 32 one-KiB pieces (request counter budget)
      p.in_ssq = k.in_ssq;
      p.in_parts = uint32_t(k.in_parts), p.in_stride = uint32_t(k.in_stride);
      p.in_eps = k.eps, p.in_inv_size = 1.0f / float(k.norm_size);
    }
    if (k.out_ssq || k.out_gamma) {
      if (a.dual || nmat != 1 || (k.out_ssq && k.out_stride < w0->ntiles)) return hipErrorInvalidValue;
      p.out_gamma = k.out_gamma, p.out_ssq = k.out_ssq, p.out_stride = uint32_t(k.out_stride);
      p.out_ovf = k.out_gamma ? kvm_overflow_word() : nullptr;
    }
  }
  if (a.rope) {
    const ns_qkv_rope& r = *a.rope;
    if ((mode != GV_MSEG && mode != GV_MSEGP) || nmat != 3 || r.mode != (neox ? 2 : 0) || r.head_size < 2 || (r.head_size & 1) || r.n_dims != r.head_size ||
        !r.kcache16 || !r.vcache16 || !r.cos_sin || r.n_past < 0 || p.mat[0].n != r.heads * r.head_size ||
        p.mat[1].n != r.heads_kv * r.head_size || p.mat[2].n != r.heads_kv * r.head_size)
      return hipErrorInvalidValue;
    p.rope.kc = static_cast<_Float16*>(r.kcache16), p.rope.vc = static_cast<_Float16*>(r.vcache16);
    p.rope.c_sl = r.cache_step_sl, p.rope.c_head = r.cache_step_head;
    p.rope.head_size = r.head_size, p.rope.n_past = r.n_past;
    p.rope.cos_sin = reinterpret_cast<const float2*>(r.cos_sin);
    p.rope.on = 1;
    if (a.rope_route) {
      const QkvRopeRoute& q = *a.rope_route;
      if (rows != 1) return hipErrorInvalidValue;
      p.rope.kmove = q.kmove, p.rope.kd_pos = q.kd_pos;
      p.rope.k32 = q.k32, p.rope.v32 = q.v32;
      p.rope.k32_head = q.k32_head, p.rope.k32_dim = q.k32_dim, p.rope.k32_tok = q.k32_tok;
      p.rope.v32_head = q.v32_head, p.rope.v32_dim = q.v32_dim, p.rope.v32_tok = q.v32_tok;
      p.rope.ovf = q.overflow;
    }
  }
  if (uint64_t(rows) * uint64_t(a.lda) * 4 >= (uint64_t(1) << 30)) return hipErrorNotSupported;  // staging offsets

  // waves per workgroup: enough waves on the chip to overlap dequantisation with the stream (as tuned for
  // smallm_kernel, profiles/r01*); the rings of a workgroup must fit in LDS beside the staged activations
  const int grid = neox ? int(tiles / 2) : int(tiles);
  const int nq = (a.dual || neox) ? 2 : 1;
  const uint32_t sbytes = uint32_t(w0->sps) * (w0->scale_dt == DT_F32 ? 4u : 2u);
  const uint32_t slot = 1024u + 16u * sbytes + (w0->asym ? 16u * uint32_t(w0->sps) : 0u);
  auto ring_bytes = [&](int waves) {  // a wave's ring: one slot per item it can have in flight, at least the reduction scratch
    const uint32_t items = ((ks + uint32_t(waves) - 1) / uint32_t(waves)) * uint32_t(nq);
    const size_t b = size_t(std::min<uint32_t>(items, uint32_t(kGvPF))) * slot;
    return std::max<size_t>((b + 15) & ~size_t(15), size_t(nq) * 1024);
  };
  // (the pair mode takes the wave count of the GV_MSEG launch of the same weights: the same split of K, the same bits)
  int nw = decode_waves(int(tiles), int(ks), a.dual);
  {
    while (nw > 1 && ((a_bytes + 15) & ~size_t(15)) + ssq_bytes + size_t(nw) * ring_bytes(nw) > kGvMaxLds) nw /= 2;
  }
  uint32_t nw_log2 = 0;
  while ((1 << nw_log2) < nw) nw_log2++;
  if (a32 && uint64_t(rows) * ((uint64_t(ks) * uint32_t(kstep) * 4u + 1023u) >> 10) > uint64_t(nw) * kGvA32Regs) {
    if (i8q) return a.i8->quantized ? hipErrorNotSupported : hipErrorNotReady;  // (quantized beforehand it fits: the caller's retry takes XV = 3)
    return hipErrorNotSupported;  // more fp32 pieces than the waves hold in registers: smallm_kernel stages those
  }

  p.ks = ks;
  p.qstride = w0->qstride;
  p.nw_log2 = nw_log2;
  p.sstride = w0->sstride;
  p.zstride = w0->zstride;
  p.srows = uint32_t(w0->srows);
  {
    int mul, shift;
    if (!srow_params(w0, &mul, &shift)) return hipErrorNotSupported;
    p.srow_mul = uint32_t(mul), p.srow_shift = uint32_t(shift);
  }
  p.m = a.m;
  p.k = w0->k;
  p.lda = i8q ? a.i8->lda32 : i8s ? a.i8->ldq : a.lda;
  p.row_stride = row_stride;
  p.ssq_off = uint32_t((a_bytes + 15) & ~size_t(15));
  p.ring_off = p.ssq_off + uint32_t(ssq_bytes);
  p.c2 = a.c2;
  p.d = a.d;
  p.ldc = a.ldc;
  p.ldd = a.ldd;
  p.epilogue = a.epilogue;
  if (w0->kind == WK_F4) f4_lut_planes(w0->lut, &p.lut);
  p.f8 = f8_consts(w0->qtype);
#ifdef NS_TRACE
  p.trace = trace_buffer();
#endif
  p.ring_stride = uint32_t(ring_bytes(nw));
  const size_t lds = size_t(p.ring_off) + size_t(nw) * p.ring_stride;
  if (lds > kGvMaxLds) return hipErrorNotSupported;
  if (moe) {
    p.moe_table = static_cast<const MoeExpertRow*>(a.moe->table);
    p.moe_id = a.moe->id;
    p.moe_n = a.moe->n_as;
    p.moe_table1 = static_cast<const MoeExpertRow*>(a.moe->table1);
    p.moe_w = a.moe->w;
    p.moe_nsel = uint32_t(a.moe->nsel);
    p.moe_sel_mul = (65536u + p.moe_nsel - 1u) / p.moe_nsel;
    p.moe_ids_stride = a.moe->ids_stride, p.moe_w_stride = a.moe->w_stride;
    p.moe_a_stride = uint32_t(a.moe->a_stride), p.moe_c_stride = uint32_t(a.moe->c_stride), p.moe_d_stride = uint32_t(a.moe->d_stride);
  }
  p.pl_bits = planes ? uint32_t(w0->pl_bits) : 0u;
  p.pl_lanes = planes ? w0->code_rec / 16u : 64u;
  const int mode_x = mode | (a32 && !moe ? kGvModeA32 : 0) | (i8s ? kGvModeI8 : 0) | (moe ? kGvModeMoe : 0) | (planes ? kGvModePlanes : 0);

  // the weight's slice (a slice the build leaves out is an undefined symbol when the library is linked)
  const int grid_y = moe ? a.moe->pairs : 1;
#define NS_SLICE(KIND, SPS) launch_gemv_##KIND##_##SPS(p, w0->scale_dt, w0->asym, mode_x, grid, nw, lds, st, grid_y)
  switch (w0->kind) {
    case WK_INT4: return w0->sps == 4 ? NS_SLICE(INT4, 4) : w0->sps == 2 ? NS_SLICE(INT4, 2) : NS_SLICE(INT4, 1);
    case WK_INT8: return w0->sps == 2 ? NS_SLICE(INT8, 2) : NS_SLICE(INT8, 1);
    case WK_F8: return w0->sps == 2 ? NS_SLICE(F8, 2) : NS_SLICE(F8, 1);
    default: return w0->sps == 4 ? NS_SLICE(F4, 4) : w0->sps == 2 ? NS_SLICE(F4, 2) : NS_SLICE(F4, 1);
  }
#undef NS_SLICE
}

void touch_gemv_module() {
#define NS_GEMV_TOUCH(KIND, SPS) touch_gemv_##KIND##_##SPS();
  NS_GEMV_SLICES(NS_GEMV_TOUCH)
#undef NS_GEMV_TOUCH
}
}  // namespace ns
