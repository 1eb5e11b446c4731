// ns_attn_decode.hip — fused attention, the kernels with one query row per workgroup, and the launch of a plan that names one (ns_attn.h).
//
// attn_kernel: one 256-thread workgroup per (query row, head, batch) — the unit the reference parallelises over
// (mha_dense_wrapper.h:1429-1432).  Keys are walked in chunks of 1024 with the online-softmax recurrence, so any
// context length runs in 4 KB of LDS:
//   scores   thread t takes keys t, t+256, ... of the chunk: fp32 dot of the (pre-scaled) query in LDS with the fp16 key
//            row (16-byte loads when the head dimension is contiguous, element strides otherwise, e.g. transposed K)
//   softmax  workgroup max / sum through LDS; running (m, l) rescale the accumulator
//   P.V      thread (d, part) accumulates output dim d over every `parts`-th key of the chunk: consecutive threads read
//            consecutive halves of a V row (coalesced); partitions are summed through LDS at the end
// fp32 throughout (the reference's NE_ATTN_FLAG_PREFER_FP32 form; its default path rounds Q, K and P to bf16 and is
// checked against this form at 1e-2 by its own tests, mha_dense_tests.cpp:147).
//
// attn_split_kernel (the fast path: contiguous head dimension, head group of 1/2/4/8): flash-decoding layout.
//   grid = (context splits, kv heads x query rows, batch).  A workgroup reads each K / V row of its context range ONCE
//   and serves all `G` query heads that share the kv head (GQA); 16 lanes x 16 B cover one row, so a wave works on 4 keys
//   and the workgroup on 16 keys at a time, each 16-lane group carrying its own online-softmax state (m, l, acc) — no
//   communication inside the loop.  States are merged by shuffles inside a wave, through LDS across waves, and across
//   splits by attn_merge_kernel (plain stores + a kernel boundary: no device-scope fences, which cost an L2 write-back
//   per XCD on MI355X).  HBM-bound on K and V: 2 * sl_kv * heads_kv * head_size * 2 B per query row.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "ns_attn.h"
#include "ns_launch.h"

namespace ns {

constexpr int kAttnChunk = 1024;

__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off, 64);
    v = is_max ? fmaxf(v, o) : v + o;
  }
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int i = 1; i < kAttnThreads / 64; i++) r = is_max ? fmaxf(r, red[i]) : r + red[i];
  return r;
}

__global__ __launch_bounds__(kAttnThreads) void attn_kernel(const AttnParams p) {
  __shared__ float q_s[256];
  __shared__ float s_s[kAttnChunk];
  __shared__ float red[kAttnThreads / 64];
  __shared__ float part_s[kAttnThreads];

  const int i = blockIdx.x, ihn = blockIdx.y, ibs = blockIdx.z;
  const int t = threadIdx.x;
  const int hs = p.head_size;
  const int ihkv = ihn / (p.head_num / p.heads_kv);
  const bool causal = (p.flags & NS_ATTN_FLAG_IS_CAUSAL) != 0;
  const bool alibi = (p.flags & NS_ATTN_FLAG_IS_ALIBI8) != 0;
  const bool tanh30 = (p.flags & NS_ATTN_FLAG_IS_TANH30) != 0;
  const int unmasked = causal ? (p.sl_kv - p.sl_q) + i + 1 : p.sl_kv;  // mha_dense_wrapper.h:1440-1441

  const float* q = p.q + ibs * p.step_q_bs + ihn * p.step_q_head_num + i * p.step_q_sl;
  const _Float16* kb = p.k + ibs * p.step_k_bs + ihkv * p.step_k_head_num;
  const _Float16* vb = p.v + ibs * p.step_v_bs + ihkv * p.step_v_head_num;
  float* dst = p.dst + ibs * p.step_dst_bs + ihn * p.step_dst_head_num + i * p.step_dst_sl;

  if (t < hs) q_s[t] = q[t] * p.qk_scale;
  float slope = 0.f;
  if (alibi)  // mha_dense_wrapper.h:1424-1447
  {
    const int gh = ihn + p.alibi_head_off;
    slope = gh < p.alibi_log2_floor ? powf(p.alibi_m0, float(gh + 1)) : powf(p.alibi_m1, float(2 * (gh - p.alibi_log2_floor) + 1));
  }
  __syncthreads();

  const int parts = kAttnThreads / p.hs_pad;  // key partitions of the P.V phase
  const int d = t % p.hs_pad, part = t / p.hs_pad;
  const bool k_vec = p.step_k_head_size == 1 && (hs & 7) == 0 && (p.step_k_sl & 7) == 0 &&
                     ((reinterpret_cast<uintptr_t>(kb) & 15) == 0);
  float m_run = -INFINITY, l_run = 0.f, acc = 0.f;

  for (int c0 = 0; c0 < unmasked; c0 += kAttnChunk) {
    const int cn = min(kAttnChunk, unmasked - c0);
    // ---- scores of this chunk ----
    float cmax = -INFINITY;
    for (int jj = t; jj < cn; jj += kAttnThreads) {
      const int j = c0 + jj;
      const _Float16* kr = kb + (long long)j * p.step_k_sl;
      float s = 0.f;
      if (k_vec) {
        typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
        for (int e = 0; e < hs; e += 8) {
          const half8_t kv = *reinterpret_cast<const half8_t*>(kr + e);
#pragma unroll
          for (int x = 0; x < 8; x++) s += q_s[e + x] * float(kv[x]);
        }
      } else {
        for (int e = 0; e < hs; e++) s += q_s[e] * float(kr[(long long)e * p.step_k_head_size]);
      }
      if (tanh30) s = 30.f * tanhf(s * (1.f / 30.f));
      s += float(j) * slope;
      s_s[jj] = s;
      cmax = fmaxf(cmax, s);
    }
    cmax = block_reduce(cmax, true, red);
    const float m_new = fmaxf(m_run, cmax);
    // ---- probabilities (unnormalised) ----
    float csum = 0.f;
    for (int jj = t; jj < cn; jj += kAttnThreads) {
      const float e = expf(s_s[jj] - m_new);
      s_s[jj] = e;
      csum += e;
    }
    csum = block_reduce(csum, false, red);  // also orders the s_s writes before the reads below
    const float resc = expf(m_run - m_new);  // exp(-inf) = 0 on the first chunk
    l_run = l_run * resc + csum;
    acc *= resc;
    m_run = m_new;
    // ---- P . V ----
    if (d < hs) {
      const _Float16* vd = vb + (long long)d * p.step_v_head_size;
      for (int jj = part; jj < cn; jj += parts) acc += s_s[jj] * float(vd[(long long)(c0 + jj) * p.step_v_sl]);
    }
    __syncthreads();  // s_s is rewritten by the next chunk
  }
  part_s[t] = acc;
  __syncthreads();
  if (t < hs) {
    float o = 0.f;
    for (int pp = 0; pp < parts; pp++) o += part_s[pp * p.hs_pad + t];
    const float y = o / l_run * p.out_scale;
    dst[t] = y;
    if (p.dst16) p.dst16[dst - p.dst + t] = (_Float16)y;
  }
}


// ---------------------------------------------------------------------------------------------------------------
// split-KV kernel
// ---------------------------------------------------------------------------------------------------------------
// stores / loads past every cache (sc0 sc1): partial results cross XCDs inside one launch
__device__ __forceinline__ void st_through(float* p, float v) {
  __hip_atomic_store(reinterpret_cast<uint32_t*>(p), __builtin_bit_cast(uint32_t, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ float ld_through(const float* p) {
  return __builtin_bit_cast(float, __hip_atomic_load(reinterpret_cast<const uint32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}

// What follows the key loop of a split kernel (attn_split_kernel and attn_stream_kernel share it): the four key groups of a wave are
// combined by shuffles, the waves through LDS (acc_s: [4 waves][G][16 * DPL] floats), then either the output row (one split) or the
// split's partial (max, sum, unnormalised output) is stored — and, with tickets, the last split of a kv head merges inside the launch.
template <int G, int DPL, int LPK = 16>  // LPK: lanes per key (64 / LPK key groups in a wave)
__device__ __forceinline__ void attn_split_finish(const AttnSplitParams& sp, float (&acc)[G][DPL], float (&m)[G], float (&lsum)[G], float* acc_s,
                                                  float (&ml_s)[4][G][2], int split, int chunk, int ihkv, int i, int ibs, int live) {
  const AttnParams& p = sp.a;
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int hs = p.head_size;
  const int d0 = (l & (LPK - 1)) * DPL;
  auto head_of = [&](int g) { return ihkv * sp.g_full + min(chunk * G + g, sp.g_full - 1); };
  auto head_live = [&](int g) { return chunk * G + g < sp.g_full; };
  // ---- merge the 4 key groups of a wave (lanes with equal dl) by shuffles ----
#pragma unroll
  for (int g = 0; g < G; g++) {
#pragma unroll
    for (int off = LPK; off <= 32; off <<= 1) {
      const float mo = __shfl_xor(m[g], off, 64), lo = __shfl_xor(lsum[g], off, 64);
      const float mn = fmaxf(m[g], mo);
      const float ca = mn == -INFINITY ? 0.f : expf(m[g] - mn), cb = mn == -INFINITY ? 0.f : expf(mo - mn);
      lsum[g] = lsum[g] * ca + lo * cb;
#pragma unroll
      for (int e = 0; e < DPL; e++) acc[g][e] = acc[g][e] * ca + __shfl_xor(acc[g][e], off, 64) * cb;
      m[g] = mn;
    }
  }
  // ---- across the 4 waves through LDS ----
  if (l < LPK) {
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (l == 0) {
        ml_s[w][g][0] = m[g];
        ml_s[w][g][1] = lsum[g];
      }
#pragma unroll
      for (int e = 0; e < DPL; e++) acc_s[(w * G + g) * LPK * DPL + d0 + e] = acc[g][e];
    }
  }
  __syncthreads();
  // thread (g, d) finishes output dim d of head g
  for (int idx = t; idx < G * LPK * DPL; idx += kAttnThreads) {
    const int g = idx / (LPK * DPL), dd = idx % (LPK * DPL);
    if (dd >= hs || !head_live(g)) continue;
    float mb = -INFINITY;
#pragma unroll
    for (int ww = 0; ww < 4; ww++) mb = fmaxf(mb, ml_s[ww][g][0]);
    float lb = 0.f, ab = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ww++) {
      const float c = ml_s[ww][g][0] == -INFINITY ? 0.f : expf(ml_s[ww][g][0] - mb);
      lb += ml_s[ww][g][1] * c;
      ab += acc_s[(ww * G + g) * LPK * DPL + dd] * c;
    }
    const int ihn = head_of(g);
    if (live == 1) {
      float* dst = p.dst + ibs * p.step_dst_bs + ihn * p.step_dst_head_num + i * p.step_dst_sl;
      const float y = ab / lb * p.out_scale;
      dst[dd] = y;
      if (p.dst16) p.dst16[dst - p.dst + dd] = (_Float16)y;
    } else {
      float* wp = sp.ws + ((((size_t)ibs * p.sl_q + i) * p.head_num + ihn) * sp.nsplit + split) * (2 + hs);
      if (sp.tickets) {
        if (dd == 0) {
          st_through(wp, mb);
          st_through(wp + 1, lb);
        }
        st_through(wp + 2 + dd, ab);
      } else {
        if (dd == 0) {
          wp[0] = mb;
          wp[1] = lb;
        }
        wp[2 + dd] = ab;
      }
    }
  }
  if (live == 1 || !sp.tickets) return;
  // ---- merge inside the launch: the write-through stores above are drained, the workgroup draws a ticket, and the one that
  // draws the last of (batch, query row, kv head) combines all splits — the sums attn_merge_kernel forms, in the same order ----
  __shared__ uint32_t drawn_s;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  uint32_t* tk = sp.tickets + (((size_t)ibs * p.sl_q + i) * p.heads_kv + ihkv) * sp.chunks + chunk;
  if (t == 0) drawn_s = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (drawn_s != uint32_t(live - 1)) return;
  if (t == 0) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // zero again for the next launch
  const int ns = live;
  for (int idx = t; idx < G * LPK * DPL; idx += kAttnThreads) {
    const int g = idx / (LPK * DPL), dd = idx % (LPK * DPL);
    if (dd >= hs || !head_live(g)) continue;
    const int ihn = head_of(g);
    const float* wq = sp.ws + (((size_t)ibs * p.sl_q + i) * p.head_num + ihn) * sp.nsplit * (2 + hs);
    float mb = -INFINITY, lb = 0.f, ab = 0.f;
    if (ns <= 16) {  // every load of the merge requested at once
      float mv[16], lv[16], ov[16];
#pragma unroll
      for (int s2 = 0; s2 < 16; s2++) {
        const bool on = s2 < ns;
        mv[s2] = on ? ld_through(wq + s2 * (2 + hs)) : -INFINITY;
        lv[s2] = on ? ld_through(wq + s2 * (2 + hs) + 1) : 0.f;
        ov[s2] = on ? ld_through(wq + s2 * (2 + hs) + 2 + dd) : 0.f;
      }
#pragma unroll
      for (int s2 = 0; s2 < 16; s2++) mb = fmaxf(mb, mv[s2]);
#pragma unroll
      for (int s2 = 0; s2 < 16; s2++) {
        if (s2 < ns) {
          const float c = mv[s2] != -INFINITY ? expf(mv[s2] - mb) : 0.f;
          lb += lv[s2] * c;
          ab += ov[s2] * c;
        }
      }
    } else {
      for (int s2 = 0; s2 < ns; s2++) mb = fmaxf(mb, ld_through(wq + s2 * (2 + hs)));
      for (int s2 = 0; s2 < ns; s2++) {
        const float ms = ld_through(wq + s2 * (2 + hs));
        const float c = ms != -INFINITY ? expf(ms - mb) : 0.f;
        lb += ld_through(wq + s2 * (2 + hs) + 1) * c;
        ab += ld_through(wq + s2 * (2 + hs) + 2 + dd) * c;
      }
    }
    float* dst = p.dst + ibs * p.step_dst_bs + ihn * p.step_dst_head_num + i * p.step_dst_sl;
    const float y = ab / lb * p.out_scale;
    dst[dd] = y;
    if (p.dst16) p.dst16[dst - p.dst + dd] = (_Float16)y;
  }
}

// Per-request form (ROWS instantiations): an idle slot — a live length of 0 — has no key to attend over; the workgroups of its first range write the
// output rows of their heads as zeros, every workgroup of the slot leaves before it has requested anything.
template <int G>
__device__ __forceinline__ void attn_zero_rows(const AttnSplitParams& sp, int chunk, int ihkv, int i, int ibs) {
  const AttnParams& p = sp.a;
  for (int idx = threadIdx.x; idx < G * p.head_size; idx += kAttnThreads) {
    const int g = idx / p.head_size, dd = idx % p.head_size;
    if (chunk * G + g >= sp.g_full) continue;
    float* dst = p.dst + ibs * p.step_dst_bs + (ihkv * sp.g_full + chunk * G + g) * p.step_dst_head_num + i * p.step_dst_sl;
    dst[dd] = 0.f;
    if (p.dst16) p.dst16[dst - p.dst + dd] = (_Float16)0.f;
  }
}

// ROWS (both split kernels and the merge): one live length per batch entry (ns_hip_attn_decode_rows, AttnPlan::rows); false: the code as without it
// PAGED (both split kernels, with ROWS): K / V are the pools of a paged cache (ns_hip_attn_decode_paged, AttnPlan::paged) — key j of request ibs is read
// from the cell attn_page_cell names; the assignment of keys to lanes and steps and the order of the softmax updates are those of the slab form, so the
// two give the same bits over the same keys.  A block id outside the pool is never turned into an address: such a key reads as zeros (its request's
// row is then whatever that gives; no other request is touched).  A PAGED kernel takes an argument block of its own (AttnPagedParams: the page
// description around AttnSplitParams); every other instantiation keeps the block, and the code, it had.
template <bool PAGED>
using AttnKernelArgs = std::conditional_t<PAGED, AttnPagedParams, AttnSplitParams>;
__device__ __forceinline__ const AttnSplitParams& attn_sp(const AttnSplitParams& kp) { return kp; }
__device__ __forceinline__ const AttnSplitParams& attn_sp(const AttnPagedParams& kp) { return kp.sp; }
__device__ __forceinline__ AttnPage attn_pg(const AttnSplitParams&) { return AttnPage{}; }
__device__ __forceinline__ const AttnPage& attn_pg(const AttnPagedParams& kp) { return kp.pg; }

template <int G, int DPL, bool ROWS = false, bool PAGED = false>  // G query heads per kv head; DPL head dims per lane (8: head_size <= 128, 16: <= 256)
__global__ __launch_bounds__(kAttnThreads) void attn_split_kernel(const AttnKernelArgs<PAGED> kp) {
  const AttnSplitParams& sp = attn_sp(kp);
  [[maybe_unused]] const AttnPage& pg = attn_pg(kp);
  const AttnParams& p = sp.a;
  __shared__ float ml_s[4][G][2];
  extern __shared__ float acc_s[];  // [4 waves][G][16 * DPL]
  const int split = sp.heads_first ? blockIdx.y : blockIdx.x;
  const int by = sp.heads_first ? blockIdx.x : blockIdx.y;
  const int chunk = by % sp.chunks, ykv = by / sp.chunks;
  const int ihkv = ykv % p.heads_kv, i = ykv / p.heads_kv, ibs = blockIdx.z;
  // query head of slot g: heads past the group's end repeat its last head (computed, never stored)
  auto head_of = [&](int g) { return ihkv * sp.g_full + min(chunk * G + g, sp.g_full - 1); };
  auto head_live = [&](int g) { return chunk * G + g < sp.g_full; };
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int kg = t >> 4;  // key group 0..15
  const int dl = l & 15;  // dim lane
  const int hs = p.head_size;
  const bool causal = (p.flags & NS_ATTN_FLAG_IS_CAUSAL) != 0;
  const bool alibi = (p.flags & NS_ATTN_FLAG_IS_ALIBI8) != 0;
  const bool tanh30 = (p.flags & NS_ATTN_FLAG_IS_TANH30) != 0;
  const int sl_kv = attn_live_kv<ROWS>(sp, ibs), live = attn_live_splits(sp, sl_kv);
  if constexpr (ROWS) {
    if (sl_kv == 0) {  // an idle slot
      if (split == 0) attn_zero_rows<G>(sp, chunk, ihkv, i, ibs);
      return;
    }
  }
  if (split >= live) return;  // (moving context length: a range past the live keys)
  const int unmasked = causal ? (sl_kv - p.sl_q) + i + 1 : sl_kv;
  const int kps = attn_live_kps(sp, sl_kv);
  const int j0 = split * kps, j1 = min(unmasked, j0 + kps);
  const int d0 = dl * DPL;
  const bool dact = d0 < hs;  // head sizes that are not a multiple of DPL are rejected by the host

  // (PAGED: p.k / p.v are the pools' bases and attn_plan has set the batch strides to 0 — a request has no slab)
  const _Float16* kb = p.k + ibs * p.step_k_bs + ihkv * p.step_k_head_num + d0;
  const _Float16* vb = p.v + ibs * p.step_v_bs + ihkv * p.step_v_head_num + d0;

  float q[G][DPL], acc[G][DPL], m[G], lsum[G], slope[G];
#pragma unroll
  for (int g = 0; g < G; g++) {
    const int ihn = head_of(g);
    const float* qp = p.q + ibs * p.step_q_bs + ihn * p.step_q_head_num + i * p.step_q_sl + d0;
#pragma unroll
    for (int e = 0; e < DPL; e++) {
      q[g][e] = dact ? qp[e] * p.qk_scale : 0.f;
      acc[g][e] = 0.f;
    }
    m[g] = -INFINITY;
    lsum[g] = 0.f;
    slope[g] = 0.f;
    if (alibi) {
      const int gh = ihn + p.alibi_head_off;
      slope[g] = gh < p.alibi_log2_floor ? powf(p.alibi_m0, float(gh + 1)) : powf(p.alibi_m1, float(2 * (gh - p.alibi_log2_floor) + 1));
    }
  }

  typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
  // U keys per thread and step: their K and V rows are requested together (a decode step of this kernel is bound by
  // the bytes in flight — 2 x 16 B per lane and step kept a CU at ~16 KiB, 2.4 TB/s at 2048 positions,
  // profiles/r02o), and one softmax update serves all U scores.
#ifndef NS_ATTN_U
#define NS_ATTN_U 4
#endif
  // NS_ATTN_DB=1 (round 4, measured and NOT adopted): two register sets, the rows of step s + 1 requested BEFORE step s is computed, half as
  // many keys per step.  The stream alone is 8.4 us of this kernel's ~10.8 (-DNS_ATTN_ABL=1), the steps' arithmetic sits between
  // their request batches — yet requesting ahead is SLOWER: split + merge 15.5 us against 14.4 on one box (profiles/r04bb_*), with 4
  // keys per step as well.  Like the decode GEMV, this kernel loses when more requests are in flight earlier.
#ifndef NS_ATTN_DB
#define NS_ATTN_DB 0
#endif
  constexpr int U0 = G * DPL <= 16 ? NS_ATTN_U : (G * DPL <= 64 ? 2 : 1);  // register budget: acc and q are G x DPL each (8: no gain)
  constexpr int U = NS_ATTN_DB ? (U0 > 1 ? U0 / 2 : 1) : U0;
  typedef half8_t KvRows[U][DPL / 8];
  auto request = [&](int jb, KvRows& kv, KvRows& vv) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int j = jb + 16 * u;
      if constexpr (PAGED) {  // the key's cell in either pool (the table entry is fetched once: the same address); -1: no access, the key reads as zeros
        long long ck = -1, cv = -1;
        if (dact && j < j1) ck = attn_page_cell(pg, ibs, j, p.step_k_sl), cv = attn_page_cell(pg, ibs, j, p.step_v_sl);
#pragma unroll
        for (int c = 0; c < DPL / 8; c++) {
          kv[u][c] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
          vv[u][c] = kv[u][c];
          if (ck >= 0 && cv >= 0) {
            kv[u][c] = __builtin_nontemporal_load(reinterpret_cast<const half8_t*>(kb + ck + 8 * c));
            vv[u][c] = __builtin_nontemporal_load(reinterpret_cast<const half8_t*>(vb + cv + 8 * c));
          }
        }
        continue;
      }
      const bool live = dact && j < j1;
#pragma unroll
      for (int c = 0; c < DPL / 8; c++) {
        kv[u][c] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
        vv[u][c] = kv[u][c];
        if (live) {
#ifndef NS_ATTN_NO_NT  // streaming (non-temporal) loads: every K / V byte is read once per token (15.5 -> 14.6 us at 2048 positions)
          kv[u][c] = __builtin_nontemporal_load(reinterpret_cast<const half8_t*>(kb + (long long)j * p.step_k_sl + 8 * c));
          vv[u][c] = __builtin_nontemporal_load(reinterpret_cast<const half8_t*>(vb + (long long)j * p.step_v_sl + 8 * c));
#else
          kv[u][c] = *reinterpret_cast<const half8_t*>(kb + (long long)j * p.step_k_sl + 8 * c);
          vv[u][c] = *reinterpret_cast<const half8_t*>(vb + (long long)j * p.step_v_sl + 8 * c);
#endif
        }
      }
    }
  };
  auto consume = [&](int jb, const KvRows& kv, const KvRows& vv) {
#if defined(NS_ATTN_ABL) && NS_ATTN_ABL == 1  // timing ablation (diagnostic builds): the K / V stream alone
#pragma unroll
    for (int u = 0; u < U; u++) acc[0][0] += float(kv[u][0][0]) + float(vv[u][0][0]);
    m[0] = 0.f, lsum[0] = 1.f;
    return;
#endif
#pragma unroll
    for (int g = 0; g < G; g++) {
      float s[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        float t2 = 0.f;
#pragma unroll
        for (int e = 0; e < DPL; e++) t2 += q[g][e] * float(kv[u][e / 8][e % 8]);
        s[u] = t2;
      }
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) {
#pragma unroll
        for (int u = 0; u < U; u++) s[u] += __shfl_xor(s[u], off, 64);
      }
      float m_new = m[g];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int j = jb + 16 * u;
        if (tanh30) s[u] = 30.f * tanhf(s[u] * (1.f / 30.f));
        s[u] += float(j) * slope[g];
        if (j >= j1) s[u] = -INFINITY;
        m_new = fmaxf(m_new, s[u]);
      }
      // jb < j1: the first of the U keys is live, so m_new is finite here
      const float corr = expf(m[g] - m_new);
      float pj[U], psum = 0.f;
#pragma unroll
      for (int u = 0; u < U; u++) {
        pj[u] = expf(s[u] - m_new);  // exp(-inf) = 0 for the keys past the end
        psum += pj[u];
      }
      lsum[g] = lsum[g] * corr + psum;
#pragma unroll
      for (int e = 0; e < DPL; e++) {
        float a2 = acc[g][e] * corr;
#pragma unroll
        for (int u = 0; u < U; u++) a2 += pj[u] * float(vv[u][e / 8][e % 8]);
        acc[g][e] = a2;
      }
      m[g] = m_new;
    }
  };
  {
    KvRows kvA, vvA, kvB, vvB;
    int jb = j0 + kg;
    if (jb < j1) request(jb, kvA, vvA);
    while (jb < j1) {
      int jn = jb + 16 * U;
      if (NS_ATTN_DB && jn < j1) request(jn, kvB, vvB);
      consume(jb, kvA, vvA);
      jb = jn;
      if (jb >= j1) break;
      jn = jb + 16 * U;
      if (NS_ATTN_DB) {
        if (jn < j1) request(jn, kvA, vvA);
        consume(jb, kvB, vvB);
      } else {
        request(jb, kvA, vvA);
        continue;
      }
      jb = jn;
    }
  }

  attn_split_finish<G, DPL>(sp, acc, m, lsum, acc_s, ml_s, split, chunk, ihkv, i, ibs, live);
}

// ---------------------------------------------------------------------------------------------------------------
// attn_stream_kernel (round 5) — attn_split_kernel's arithmetic on the decode GEMV's streaming skeleton (ns_gemv.hip): the K and V rows
// of the workgroup's context range go HBM -> LDS by DMA (buffer_load ... lds, 16 B per lane, non-temporal) into a PRIVATE ring per
// wave, every request of the range in flight before the first key is multiplied; the lanes then read back exactly the 16 bytes they
// requested (lane-linear image: no bank conflicts, no staging registers held across the memory round trip) behind hand-counted
// s_waitcnt vmcnt.  What this changes against attn_split_kernel: that kernel holds U = 4 keys per lane in registers, so a range of
// 128 keys is two dependent round trips of 32 KiB per workgroup (the stream alone is 8.4 of its 10.8 us at 2048 positions,
// profiles/r04bb_*); here a workgroup has its whole range — 64 KiB at 128 keys — requested within the first few hundred cycles.
// Same key -> lane mapping (wave w, step u: keys j0 + 16 u + 4 w .. + 3, lane group l >> 4 one key each, lane l & 15 eight head
// dims), same U-key softmax update, same finish (attn_split_finish); the two kernels split a context differently (own range rule below) and hipcc contracts
// their sums differently, so their outputs agree to fp32 rounding (2e-6 relative, tests/test_gpu_attention.py), not bit for bit.
// A step = 4 keys = one 1 KiB request of K + one of V per wave; ring of kAsSteps steps per wave (refilled behind the reads for longer
// ranges).  Rows past the range's end lie outside the buffer descriptor (the DMA writes zeros for them); their scores are masked and
// their V is selected to zero as in attn_split_kernel, so nothing depends on what such a slot holds.
#ifndef NS_AS_ABL
#define NS_AS_ABL 0  // timing ablations (diagnostic builds, wrong results): 1 no arithmetic in the key loop, 2 nothing behind the key loop, 3 no key loop at all (nothing streamed), 4 streamed but never read
#endif
// PAGED.  A wave's keys of one step are KPW <= 8 consecutive keys, a block holds 16 or more: they lie in at most two blocks, whatever the range's
// start.  Both table entries of a step are wave-uniform and fetched by scalar loads (the scalar cache, counted by lgkmcnt: the hand-counted vmcnt
// of the stream is untouched, and a refill's entries are requested one batch ahead, in front of the wait that batch has anyway); every lane picks
// its key's block of the two and forms its offset into ONE descriptor that spans the pool.  A key at or behind the range's end, and a key whose
// block id is not a block of the pool, gets the offset pool_bytes — outside the descriptor, so it fetches nothing.  The dependent load in front of
// the stream is the price of the translation (docs/kernels/attention.md, "Decode over a paged cache").
template <int G, int LPK = 16, bool ROWS = false, bool PAGED = false>  // LPK lanes per key: 16 (head sizes 72 .. 128) or 8 (40 .. 64: a 1 KiB request then holds 8 key rows, a wave step 8 keys)
__global__ __launch_bounds__(kAttnThreads) void attn_stream_kernel(const AttnKernelArgs<PAGED> kp) {
  const AttnSplitParams& sp = attn_sp(kp);
  [[maybe_unused]] const AttnPage& pg = attn_pg(kp);
  constexpr int DPL = 8;
  constexpr int KPW = 64 / LPK;  // keys per wave and step
  constexpr int KPS = 4 * KPW;   // keys per workgroup and step
  const AttnParams& p = sp.a;
  __shared__ float ml_s[4][G][2];
  extern __shared__ __attribute__((aligned(16))) unsigned char ring_s[];  // [4 waves][kAsSteps][K image 1 KiB | V image 1 KiB]; afterwards acc_s
  typedef __attribute__((address_space(3))) unsigned char* LdsPtr;
  const int split = sp.heads_first ? blockIdx.y : blockIdx.x;
  const int by = sp.heads_first ? blockIdx.x : blockIdx.y;
  const int chunk = by % sp.chunks, ykv = by / sp.chunks;
  const int ihkv = ykv % p.heads_kv, i = ykv / p.heads_kv, ibs = blockIdx.z;
  auto head_of = [&](int g) { return ihkv * sp.g_full + min(chunk * G + g, sp.g_full - 1); };
  const int t = threadIdx.x, l = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int dl = l & (LPK - 1);
  const int hs = p.head_size;
  const bool causal = (p.flags & NS_ATTN_FLAG_IS_CAUSAL) != 0;
  const bool alibi = (p.flags & NS_ATTN_FLAG_IS_ALIBI8) != 0;
  const bool tanh30 = (p.flags & NS_ATTN_FLAG_IS_TANH30) != 0;
  const int sl_kv = attn_live_kv<ROWS>(sp, ibs), live = attn_live_splits(sp, sl_kv);
  if constexpr (ROWS) {
    if (sl_kv == 0) {  // an idle slot
      if (split == 0) attn_zero_rows<G>(sp, chunk, ihkv, i, ibs);
      return;
    }
  }
  if (split >= live) return;  // (moving context length: a range past the live keys)
  const int unmasked = causal ? (sl_kv - p.sl_q) + i + 1 : sl_kv;
  const int kps = attn_live_kps(sp, sl_kv);
  const int j0 = split * kps, j1 = min(unmasked, j0 + kps);
  const int d0 = dl * DPL;
  const bool dact = d0 < hs;
  constexpr int U = G * DPL <= 16 ? 4 : 2;  // keys per lane and softmax update: attn_split_kernel's rule (the update order decides the bits)
  static_assert(kAsSteps % U == 0, "a batch of U steps never wraps inside the ring");
  const int nsteps = NS_AS_ABL == 3 ? 0 : j1 > j0 ? (((j1 - j0 + KPS - 1) / KPS) + U - 1) / U * U : 0;  // whole batches: steps past the end fetch nothing (outside the descriptor)

  // ---- 0. the query rows are requested first (ordinary loads, OLDER than the stream: loads return in order, a row requested behind the
  //      ring would be usable only when the whole ring has landed) ----
  //      Written by hand: for a load it knows hipcc waits with vmcnt(0) at the first use, i.e. for the whole ring (it does not count
  //      the LDS-DMA requests behind it); the counted wait is in step 2.
  // PAGED: the two table entries of wave step s (clamped to the table row: steps past the range's end fetch nothing anyway).  An asm, so that it is
  // a scalar load whatever hipcc can prove of the table; its results are used behind an s_waitcnt lgkmcnt(0) only (the "+s" constraints behind each wait).
  const int tshift = PAGED ? pg.block_shift : 0;
  const int* trow = PAGED ? pg.table + (long long)ibs * pg.table_stride : nullptr;
  auto fetch_ids = [&](int s, int& ba, int& bb) {
    const int a = j0 + KPS * s + KPW * w;
    const int ea = min(a >> tshift, pg.table_stride - 1), eb = min((a + KPW - 1) >> tshift, pg.table_stride - 1);
    // (the addresses are wave-uniform, said explicitly; the halves go through uint32_t: readfirstlane returns an int, and a low half with bit 31
    // set must not be sign-extended into the high one)
    auto uniform64 = [](const int* ptr) {
      const uint64_t v = reinterpret_cast<uint64_t>(ptr);
      const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(v)), hi = __builtin_amdgcn_readfirstlane(uint32_t(v >> 32));
      return (uint64_t(hi) << 32) | lo;
    };
    const uint64_t ua = uniform64(trow + ea), ub = uniform64(trow + eb);
    asm volatile("s_load_dword %0, %1, 0x0" : "=s"(ba) : "s"(ua) : "memory");
    asm volatile("s_load_dword %0, %1, 0x0" : "=s"(bb) : "s"(ub) : "memory");
  };
  int ida[kAsSteps], idb[kAsSteps];
  if constexpr (PAGED) {
#pragma unroll
    for (int s = 0; s < kAsSteps; s++) fetch_ids(s, ida[s], idb[s]);
  }
  typedef float f4_t __attribute__((ext_vector_type(4)));
  f4_t qa[G], qb[G];
#pragma unroll
  for (int g = 0; g < G; g++) {
    // (no branch around the asm and no other definition of its outputs: hipcc takes an asm's outputs for complete and would copy
    // them — e.g. to merge them with a zero — while the data is still on its way; lanes past the head size load dims 0..7, unused)
    const float* qp = p.q + ibs * p.step_q_bs + head_of(g) * p.step_q_head_num + i * p.step_q_sl + (dact ? d0 : 0);
    asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:16" : "=&v"(qa[g]), "=&v"(qb[g]) : "v"(qp) : "memory");
  }
  __builtin_amdgcn_sched_barrier(0);
  // ---- 1. the whole range (up to the ring's depth) is requested before anything else is touched ----
  // (PAGED: the descriptors span the pools — attn_plan gives this kernel only pools of less than 4 GiB, attn_page_in32)
  const uint32_t pool_bytes = PAGED ? uint32_t(size_t(pg.pool_blocks) * size_t(pg.block_step) * 2) : 0u;
  const _Float16* kh = PAGED ? p.k : p.k + ibs * p.step_k_bs + ihkv * p.step_k_head_num;
  const _Float16* vh = PAGED ? p.v : p.v + ibs * p.step_v_bs + ihkv * p.step_v_head_num;
  const uint32_t k_bytes = PAGED ? pool_bytes : j1 > j0 ? uint32_t((size_t(j1 - 1) * p.step_k_sl + hs) * 2) : 0u;
  const uint32_t v_bytes = PAGED ? pool_bytes : j1 > j0 ? uint32_t((size_t(j1 - 1) * p.step_v_sl + hs) * 2) : 0u;
  // (the descriptors are wave-uniform; said explicitly, or hipcc wraps every request into a readfirstlane loop)
  auto uniform_ptr = [](const _Float16* ptr) {
    const uint64_t v = reinterpret_cast<uint64_t>(ptr);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(v)), hi = __builtin_amdgcn_readfirstlane(uint32_t(v >> 32));
    return reinterpret_cast<_Float16*>((uint64_t(hi) << 32) | lo);
  };
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(kh), 0, __builtin_amdgcn_readfirstlane(k_bytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(vh), 0, __builtin_amdgcn_readfirstlane(v_bytes), 0x00020000);
  const uint32_t key_l = uint32_t(j0 + KPW * w + l / LPK);  // this lane's key of step 0
  const uint32_t k_voff = (key_l * uint32_t(p.step_k_sl) + uint32_t(d0)) * 2u, k_step = uint32_t(KPS) * uint32_t(p.step_k_sl) * 2u;
  const uint32_t v_voff = (key_l * uint32_t(p.step_v_sl) + uint32_t(d0)) * 2u, v_step = uint32_t(KPS) * uint32_t(p.step_v_sl) * 2u;
  const LdsPtr ring = (LdsPtr)(ring_s) + w * (kAsSteps * 2048);
  auto issue = [&](int s) {  // step s -> slot s % kAsSteps; the key offset is part of the per-lane offset (the part the descriptor checks)
#if defined(__HIP_DEVICE_COMPILE__)
    const LdsPtr dst = ring + (s & (kAsSteps - 1)) * 2048;
    if (dact) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, reinterpret_cast<__attribute__((address_space(3))) void*>(dst), 16, k_voff + uint32_t(s) * k_step, 0, 0, 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, reinterpret_cast<__attribute__((address_space(3))) void*>(dst + 1024), 16, v_voff + uint32_t(s) * v_step, 0, 0, 2);
    }
#endif
  };
  // PAGED: step s with its two table entries — the lane's key, its block of the two, its cell through attn_page_at
  auto issue_paged = [&](int s, int ba, int bb) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int a = j0 + KPS * s + KPW * w, key = a + l / LPK;
    const int blk = (key >> tshift) == (a >> tshift) ? ba : bb;
    const long long ck = attn_page_at(pg, blk, key, p.step_k_sl), cv = attn_page_at(pg, blk, key, p.step_v_sl);
    const bool on = key < j1 && ck >= 0;
    const uint32_t ko = on ? uint32_t(ck + ihkv * p.step_k_head_num + d0) * 2u : pool_bytes;
    const uint32_t vo = on ? uint32_t(cv + ihkv * p.step_v_head_num + d0) * 2u : pool_bytes;
    const LdsPtr dst = ring + (s & (kAsSteps - 1)) * 2048;
    if (dact) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, reinterpret_cast<__attribute__((address_space(3))) void*>(dst), 16, ko, 0, 0, 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, reinterpret_cast<__attribute__((address_space(3))) void*>(dst + 1024), 16, vo, 0, 0, 2);
    }
#endif
  };
  if constexpr (PAGED) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < kAsSteps; s++) asm volatile("" : "+s"(ida[s]), "+s"(idb[s]));  // (uses stay behind the wait)
#pragma unroll
    for (int s = 0; s < kAsSteps; s++)
      if (s < nsteps) issue_paged(s, ida[s], idb[s]);
  } else {
#pragma unroll
    for (int s = 0; s < kAsSteps; s++)
      if (s < nsteps) issue(s);
  }
  __builtin_amdgcn_sched_barrier(0);

  // ---- 2. the query rows' first use (their wait is counted: the stream's requests are younger and stay in flight) ----
  switch (min(nsteps, kAsSteps)) {  // requests issued behind the query loads: two per step
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
  }
  static_assert(kAsSteps == 8, "the cases above");
  float q[G][DPL], acc[G][DPL], m[G], lsum[G], slope[G];
#pragma unroll
  for (int g = 0; g < G; g++) {
    const int ihn = head_of(g);
    asm volatile("" : "+v"(qa[g]), "+v"(qb[g]));  // (uses of the rows stay behind the wait)
#pragma unroll
    for (int e = 0; e < DPL; e++) {
      q[g][e] = dact ? (e < 4 ? qa[g][e & 3] : qb[g][e & 3]) * p.qk_scale : 0.f;
      acc[g][e] = 0.f;
    }
    m[g] = -INFINITY;
    lsum[g] = 0.f;
    slope[g] = 0.f;
    if (alibi) {
      const int gh = ihn + p.alibi_head_off;
      slope[g] = gh < p.alibi_log2_floor ? powf(p.alibi_m0, float(gh + 1)) : powf(p.alibi_m1, float(2 * (gh - p.alibi_log2_floor) + 1));
    }
  }

  typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
  typedef uint32_t u4_t __attribute__((ext_vector_type(4)));
  const uint32_t lane_lds = uint32_t(reinterpret_cast<uintptr_t>(ring)) + uint32_t(l) * 16u;
  // at most `younger` STEPS requested after the batch about to be read are still in flight (two requests per step)
  auto wait_steps = [&](int younger) {
    switch (younger) {
      case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
      case 1: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
      case 2: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
      case 3: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
      case 4: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
      case 5: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    }
  };
  for (int s0 = 0; s0 < nsteps; s0 += U) {
    int ra[U], rb[U];  // PAGED: the table entries of the steps this batch's slots are refilled with, requested in front of the batch's own wait
    if constexpr (PAGED) {
#pragma unroll
      for (int u = 0; u < U; u++) fetch_ids(s0 + kAsSteps + u, ra[u], rb[u]);
    }
    wait_steps(min(nsteps - s0 - U, kAsSteps - U));
    if (NS_AS_ABL == 4) {
#pragma unroll
      for (int u = 0; u < U; u++)
        if (s0 + kAsSteps + u < nsteps) issue(s0 + kAsSteps + u);
      continue;
    }
    u4_t kr[U], vr[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t a = lane_lds + uint32_t((s0 + u) & (kAsSteps - 1)) * 2048u;
      asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024" : "=&v"(kr[u]), "=&v"(vr[u]) : "v"(a) : "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int u = 0; u < U; u++) asm volatile("" : "+v"(kr[u]), "+v"(vr[u]));  // (uses stay behind the wait)
    __builtin_amdgcn_sched_barrier(0);
    // the slots are free: the steps one ring ahead are requested before this batch is multiplied
    if constexpr (PAGED) {
#pragma unroll
      for (int u = 0; u < U; u++) asm volatile("" : "+s"(ra[u]), "+s"(rb[u]));  // (behind the lgkmcnt(0) above: the entries have arrived)
#pragma unroll
      for (int u = 0; u < U; u++)
        if (s0 + kAsSteps + u < nsteps) issue_paged(s0 + kAsSteps + u, ra[u], rb[u]);
    } else {
#pragma unroll
      for (int u = 0; u < U; u++)
        if (s0 + kAsSteps + u < nsteps) issue(s0 + kAsSteps + u);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (NS_AS_ABL == 1) {
      acc[0][0] += __builtin_bit_cast(float, kr[0].x ^ vr[U - 1].y);
      continue;
    }
    const int jb = j0 + KPS * s0 + KPW * w + l / LPK;
    // rows past the range's end and lanes past the head size count as zeros, as attn_split_kernel's unrequested registers do
    half8_t kv[U], vv[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const bool live = dact && jb + KPS * u < j1;
      const u4_t zero = {0u, 0u, 0u, 0u};
      kv[u] = __builtin_bit_cast(half8_t, live ? kr[u] : zero);
      vv[u] = __builtin_bit_cast(half8_t, live ? vr[u] : zero);
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
      float s[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        float t2 = 0.f;
#pragma unroll
        for (int e = 0; e < DPL; e++) t2 += q[g][e] * float(kv[u][e]);
        s[u] = t2;
      }
#pragma unroll
      for (int off = LPK / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int u = 0; u < U; u++) s[u] += __shfl_xor(s[u], off, 64);
      }
      float m_new = m[g];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int j = jb + KPS * u;
        if (tanh30) s[u] = 30.f * tanhf(s[u] * (1.f / 30.f));
        s[u] += float(j) * slope[g];
        if (j >= j1) s[u] = -INFINITY;
        m_new = fmaxf(m_new, s[u]);
      }
      // a lane group whose keys of this batch are all past the end keeps m = -inf: then m_new = -inf and exp(-inf - -inf) would be NaN
      const float corr = m_new == -INFINITY ? 1.f : expf(m[g] - m_new);
      float pj[U], psum = 0.f;
#pragma unroll
      for (int u = 0; u < U; u++) {
        pj[u] = m_new == -INFINITY ? 0.f : expf(s[u] - m_new);
        psum += pj[u];
      }
      lsum[g] = lsum[g] * corr + psum;
#pragma unroll
      for (int e = 0; e < DPL; e++) {
        float a2 = acc[g][e] * corr;
#pragma unroll
        for (int u = 0; u < U; u++) a2 += pj[u] * float(vv[u][e]);
        acc[g][e] = a2;
      }
      m[g] = m_new;
    }
  }
  if (NS_AS_ABL == 2) {
    if (acc[0][0] == 123.456f) p.dst[0] = acc[0][1] + m[0] + lsum[0];
    return;
  }
  __syncthreads();  // every wave has left its ring: its first bytes become attn_split_finish's acc_s
  attn_split_finish<G, DPL, LPK>(sp, acc, m, lsum, reinterpret_cast<float*>(ring_s), ml_s, split, chunk, ihkv, i, ibs, live);
}

// one workgroup per (batch, query row, head): combine the splits' (m, l, acc).  The per-split (m, l) are fetched by
// one thread each (one round trip instead of nsplit dependent ones), the weights exp(m_s - m) go through LDS, and the
// accumulator columns are summed with independent loads.
template <bool ROWS = false>
__global__ __launch_bounds__(128) void attn_merge_kernel(const AttnSplitParams sp) {
  const AttnParams& p = sp.a;
  __shared__ float c_s[64];
  __shared__ float l_s[64];
  const int ihn = blockIdx.x, i = blockIdx.y, ibs = blockIdx.z;
  const int hs = p.head_size, t = threadIdx.x;
  const int ns = attn_live_splits(sp, attn_live_kv<ROWS>(sp, ibs));  // ns <= 64
  if (sp.kmove && ns == 1) return;  // (a single live range wrote the output row itself)
  const float* wp = sp.ws + (((size_t)ibs * p.sl_q + i) * p.head_num + ihn) * sp.nsplit * (2 + hs);
  // the common decode shapes (<= 32 splits, one output element per thread): every thread fetches all (max, sum) pairs — wave-
  // uniform addresses, scalar loads — and its own column of the partial outputs in ONE batch of loads, then merges in registers:
  // one memory round trip behind the kernel boundary instead of two with a workgroup barrier between them (round 4: the launch
  // is 4.9 us for a few KB of work; the same sums in the same order as the general form below).  Round 5: also for 17 .. 32 splits
  // (the LDS-ring kernel splits a kv head shared by 4 query heads into 32 ranges at 2048 positions).
  auto fast = [&](auto n_c) {
    constexpr int N = decltype(n_c)::value;
    float mv[N], lv[N], ov[N];
#pragma unroll
    for (int s2 = 0; s2 < N; s2++) {
      const bool on = s2 < ns;
      mv[s2] = on ? wp[s2 * (2 + hs)] : -INFINITY;
      lv[s2] = on ? wp[s2 * (2 + hs) + 1] : 0.f;
      ov[s2] = (on && t < hs) ? wp[s2 * (2 + hs) + 2 + t] : 0.f;
    }
    float mb2 = -INFINITY;
#pragma unroll
    for (int s2 = 0; s2 < N; s2++) mb2 = fmaxf(mb2, mv[s2]);
    float lb2 = 0.f, ab2 = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < N; s2++) {
      if (s2 < ns) {
        const float c = mv[s2] != -INFINITY ? expf(mv[s2] - mb2) : 0.f;
        lb2 += lv[s2] * c;
        ab2 += ov[s2] * c;
      }
    }
    if (t < hs) {
      float* dst2 = p.dst + ibs * p.step_dst_bs + ihn * p.step_dst_head_num + i * p.step_dst_sl;
      const float y = ab2 / lb2 * p.out_scale;
      dst2[t] = y;
      if (p.dst16) p.dst16[dst2 - p.dst + t] = (_Float16)y;
    }
  };
  if (ns <= 16 && hs <= int(blockDim.x)) return fast(std::integral_constant<int, 16>{});
  if (ns <= 32 && hs <= int(blockDim.x)) return fast(std::integral_constant<int, 32>{});
  float ms = -INFINITY, ls = 0.f;
  if (t < ns) {
    ms = wp[t * (2 + hs)];
    ls = wp[t * (2 + hs) + 1];
  }
  float mb = ms;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mb = fmaxf(mb, __shfl_xor(mb, off, 64));  // splits live in wave 0 (ns <= 64)
  if (t < 64) {
    c_s[t] = (t < ns && ms != -INFINITY) ? expf(ms - mb) : 0.f;
    l_s[t] = ls;
  }
  __syncthreads();
  float lb = 0.f;
  for (int s = 0; s < ns; s++) lb += l_s[s] * c_s[s];
  float* dst = p.dst + ibs * p.step_dst_bs + ihn * p.step_dst_head_num + i * p.step_dst_sl;
  for (int d = t; d < hs; d += blockDim.x) {
    float ab = 0.f;
#pragma unroll 8
    for (int s = 0; s < ns; s++) ab += wp[s * (2 + hs) + 2 + d] * c_s[s];
    const float y = ab / lb * p.out_scale;
    dst[d] = y;
    if (p.dst16) p.dst16[dst - p.dst + d] = (_Float16)y;
  }
}

// ---- launch of a plan (ns_attn_plan.cpp) -------------------------------------------------------------------------------------------------
template <int G>
static hipError_t launch_paged_g(const AttnPlan& pl, const AttnSplitParams& sp, hipStream_t st) {
  const AttnPagedParams pp = {sp, pl.page};
  if (pl.path == AP_RING)
    return pl.lpk == 16 ? launch_lds<attn_stream_kernel<G, 16, true, true>>(int(kAsLdsBytes), pl.grid, pl.block, pl.lds, st, pp)
                        : launch_lds<attn_stream_kernel<G, 8, true, true>>(int(kAsLdsBytes), pl.grid, pl.block, pl.lds, st, pp);
  if (pl.dpl == 8) {
    hipLaunchKernelGGL((attn_split_kernel<G, 8, true, true>), pl.grid, pl.block, pl.lds, st, pp);
  } else {
    hipLaunchKernelGGL((attn_split_kernel<G, 16, true, true>), pl.grid, pl.block, pl.lds, st, pp);
  }
  return hipGetLastError();
}
static hipError_t launch_paged(const AttnPlan& pl, const AttnSplitParams& sp, hipStream_t st) {
  return pl.G == 1   ? launch_paged_g<1>(pl, sp, st)
         : pl.G == 2 ? launch_paged_g<2>(pl, sp, st)
         : pl.G == 4 ? launch_paged_g<4>(pl, sp, st)
                     : launch_paged_g<8>(pl, sp, st);
}
template <int G, bool ROWS>
static hipError_t launch_split_g(const AttnPlan& pl, const AttnSplitParams& sp, hipStream_t st) {
  if (pl.path == AP_RING)  // head sizes 72 .. 128: sixteen lanes per key, 40 .. 64: eight
    return pl.lpk == 16 ? launch_lds<attn_stream_kernel<G, 16, ROWS>>(int(kAsLdsBytes), pl.grid, pl.block, pl.lds, st, sp)
                        : launch_lds<attn_stream_kernel<G, 8, ROWS>>(int(kAsLdsBytes), pl.grid, pl.block, pl.lds, st, sp);
  if (pl.dpl == 8) {
    hipLaunchKernelGGL((attn_split_kernel<G, 8, ROWS>), pl.grid, pl.block, pl.lds, st, sp);
  } else {
    hipLaunchKernelGGL((attn_split_kernel<G, 16, ROWS>), pl.grid, pl.block, pl.lds, st, sp);
  }
  return hipGetLastError();
}
template <bool ROWS>
static hipError_t launch_split(const AttnPlan& pl, const AttnSplitParams& sp, hipStream_t st) {
  return pl.G == 1   ? launch_split_g<1, ROWS>(pl, sp, st)
         : pl.G == 2 ? launch_split_g<2, ROWS>(pl, sp, st)
         : pl.G == 4 ? launch_split_g<4, ROWS>(pl, sp, st)
                     : launch_split_g<8, ROWS>(pl, sp, st);
}
// ws: the partials (pl.partial_bytes); tickets: the stream's ticket buffer when the plan wants one, nullptr = the merge launch
hipError_t launch_attn_onerow(const AttnPlan& pl, float* ws, uint32_t* tickets, hipStream_t st) {
  const AttnParams& p = pl.sp.a;
  if (pl.path == AP_GENERIC) {
    hipLaunchKernelGGL(attn_kernel, pl.grid, pl.block, 0, st, p);
    return hipGetLastError();
  }
  AttnSplitParams sp = pl.sp;
  sp.ws = ws, sp.tickets = tickets;
  hipError_t e = pl.paged ? launch_paged(pl, sp, st) : pl.rows ? launch_split<true>(pl, sp, st) : launch_split<false>(pl, sp, st);
  if (e != hipSuccess) return e;
  if (sp.nsplit > 1 && !sp.tickets) e = launch_attn_merge(sp, pl.grid.z, st, pl.rows);  // (grid.z: the batch)
  return e;
}
hipError_t launch_attn_merge(const AttnSplitParams& sp, unsigned batch, hipStream_t st, bool rows) {
  if (rows) {
    hipLaunchKernelGGL(attn_merge_kernel<true>, dim3(unsigned(sp.a.head_num), unsigned(sp.a.sl_q), batch), dim3(128), 0, st, sp);
  } else {
    hipLaunchKernelGGL(attn_merge_kernel<false>, dim3(unsigned(sp.a.head_num), unsigned(sp.a.sl_q), batch), dim3(128), 0, st, sp);
  }
  return hipGetLastError();
}

void touch_attn_module() {  // (one kernel of every attention file: each has a code object of its own)
  touch_kernel(reinterpret_cast<const void*>(attn_merge_kernel<false>));
  touch_attn_rows_module();
  touch_attn_block_module();
  touch_kvcache_module();
}

}  // namespace ns
