// ns_attn_onerow.h — device code the one-row split kernels share (internal): ns_attn_decode.hip (fp16 K / V) and ns_attn_decode_f8.hip (E4M3 pools).
// What follows a split kernel's key loop (attn_split_finish), the zero rows of an idle slot, the stores that cross XCDs inside one launch, and the
// argument block of the PAGED instantiations.  Included by kernel files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "ns_attn.h"

namespace ns {

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

template <bool PAGED>
using AttnKernelArgs = std::conditional_t<PAGED, AttnPagedParams, AttnSplitParams>;
__device__ __forceinline__ const AttnSplitParams& attn_sp(const AttnSplitParams& kp) { return kp; }
__device__ __forceinline__ const AttnSplitParams& attn_sp(const AttnPagedParams& kp) { return kp.sp; }
__device__ __forceinline__ AttnPage attn_pg(const AttnSplitParams&) { return AttnPage{}; }
__device__ __forceinline__ const AttnPage& attn_pg(const AttnPagedParams& kp) { return kp.pg; }

}  // namespace ns
