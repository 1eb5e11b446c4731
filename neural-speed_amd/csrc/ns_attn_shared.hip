// ns_attn_shared.hip — shared-prefix (cascade) decode over a paged KV cache: the kernels of ns_hip_attn_decode_paged_shared and the launch of its plan
// (attn_shared_paged_plan, ns_attn_plan.cpp; argument block AttnSharedParams, ns_attn.h).  One query row per request; the caller names groups of
// requests whose first P_g keys are the same cells.  The keys of a group's prefix are streamed ONCE per 64 (member, query head) slots and context range
// through the leader's table row, each member's own keys behind the prefix through its own row, and one merge sums both kinds of partial record.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "ns_attn.h"

namespace ns {

typedef _Float16 shalf8_t __attribute__((ext_vector_type(8)));
typedef _Float16 shalf4_t __attribute__((ext_vector_type(4)));
typedef _Float16 shalf2_t __attribute__((ext_vector_type(2)));
typedef float sfloatx4 __attribute__((ext_vector_type(4)));

// ============================================================================================================
// attn_shared_kernel — the loop of attn_block_split_kernel<HS, true> (ns_attn_block.hip: the 16x16x32 f16 MFMA operand layout, S^T = K.Q^T with 16-byte
// contiguous operands, the lane-held probabilities as the A operand of P.V, V^T staged through LDS once per block and workgroup, K / V and the table
// entries requested one block ahead, the exp2-domain online softmax, the (m ln 2, l, acc) record), repeated here with a geometry of its own:
//   PHASE 0, prefix   a workgroup is (kv head, slot block, range, GROUP): grid (slot blocks * heads_kv, nsp, groups).  slot = member * g_full + j is the
//             query row of request first + member, query head ihkv * g_full + j.  A lane derives from its slot its request, its Q row, its key limit
//             min(P_g, len_b) — per slot: a member may be shorter than the prefix, or idle — and the record it writes.  No causal limit.  The "whole block
//             visible" fast path is the wave-uniform test block end <= the least limit of the wave's live slots.  K / V addresses come from the LEADER's
//             table row only; the fetch clamp and the zero fill of V^T are tied to the largest limit of the slot block (behind it the prefix cells may
//             hold anything; below it they are some member's live keys).
//   PHASE 1, suffix   a workgroup is (kv head, slot block of ONE member, range, member): grid (slot blocks * heads_kv, nss, groups * max_group).  Slots
//             are the member's query heads j < g_full; keys [P_g + range) through the member's own row; masking, the fetch clamp and the zero fill are
//             tied to len_b.
//   both      A wave none of whose 16 slots is live fetches no K and skips its MFMAs and its softmax, but keeps staging V and keeps every barrier.
//             Slots past the live ones of a live wave compute on the last live slot's Q and never store.  A workgroup at or past its live range count,
//             of an empty group, of a member the group does not have, of a member without a key behind the prefix, or of a slot block past the slots
//             leaves before any barrier and writes nothing; a live range in which a slot saw no key writes (-inf, 0, zeros) for that slot.
// 256 threads; wave w owns slots 16w .. 16w + 15 of the block.  Ranges start at multiples of 16 (ns_attn.h), so score tile t of a block (16 keys; also
// the 16 positions of V that wave t stages) lies in ONE page: ids[t], workgroup-uniform, -1 for a tile that starts at or behind the fetch limit.
// ============================================================================================================
template <int HS, int PHASE>
__global__ __launch_bounds__(256) void attn_shared_kernel(const AttnSharedParams sp) {
  constexpr int NJ = HS / 32, NDT = HS / 16, CH = HS / 8;  // k-slices of QK^T, output column tiles, V halves per thread
  constexpr int REC = 2 + HS;                              // floats per partial record
  constexpr int NT = kBlkKB / 16, NH = kBlkKB / 32;        // score tiles, 32-deep P.V slices per block
  __shared__ __attribute__((aligned(16))) _Float16 vt[HS * kBlkVStr];
  const AttnParams& p = sp.a;
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63, nn = l & 15, g = l >> 4;
  const int ihkv = int(blockIdx.x) % p.heads_kv, sblk = int(blockIdx.x) / p.heads_kv;
  const int split = blockIdx.y;
  const int group = PHASE == 0 ? int(blockIdx.z) : int(blockIdx.z) / sp.max_group;
  const int member = PHASE == 0 ? 0 : int(blockIdx.z) % sp.max_group;
  const AttnSharedGroup gr = attn_shared_group(sp, group);
  if (member >= gr.n) return;  // an empty group, or a member the group does not have
  const int g_full = sp.g_full, nslots = PHASE == 0 ? gr.n * g_full : g_full;
  if (sblk * 64 >= nslots) return;
  const int P = gr.prefix;
  const int own_len = PHASE == 0 ? 0 : attn_shared_len(sp, gr.first + member);
  const AttnBlockLive lv = PHASE == 0 ? attn_block_live(P, sp.nsp, sp.kps_p, sp.min_keys) : attn_block_live(own_len - P, sp.nss, sp.kps_s, sp.min_keys);
  if (split >= lv.live) return;  // not a live range (an idle member, a member without a key behind the prefix): the merge reads lv.live records
  // the key limit of a slot of this block, and the largest of them: workgroup-uniform, every wave finds it for itself
  auto limit_of = [&](int slot) {
    if constexpr (PHASE == 0) return min(P, attn_shared_len(sp, gr.first + slot / g_full));
    return own_len;
  };
  int kv_lim = own_len;
  if constexpr (PHASE == 0) {
    kv_lim = sblk * 64 + l < nslots ? limit_of(sblk * 64 + l) : 0;
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) kv_lim = max(kv_lim, __shfl_xor(kv_lim, o2, 64));
    kv_lim = __builtin_amdgcn_readfirstlane(kv_lim);
  }
  const int range_begin = (PHASE == 0 ? 0 : P) + split * lv.kps;
  const int range_end = min(range_begin + lv.kps, kv_lim);
  const int table_row = gr.first + member;  // (PHASE 0: the leader)
  auto record = [&](int slot) {  // of a live slot, for this range
    const int b = gr.first + (PHASE == 0 ? slot / g_full : member), head = ihkv * g_full + (PHASE == 0 ? slot % g_full : slot);
    return sp.ws + (((size_t)b * p.head_num + head) * sp.rec_stride + (PHASE == 0 ? 0 : sp.suf_off) + split) * REC;
  };
  if (range_begin >= kv_lim) {  // (PHASE 0 only) no slot of this block sees a key of this live range: the merge still reads every record
    for (int e = tid; e < 64 * REC; e += 256) {
      const int slot = sblk * 64 + e / REC, c = e % REC;
      if (slot < nslots) record(slot)[c] = c == 0 ? -INFINITY : 0.f;
    }
    return;
  }
  const _Float16* kb = p.k + ihkv * p.step_k_head_num;  // the pools
  const _Float16* vb = p.v + ihkv * p.step_v_head_num;
  const int slot0 = sblk * 64 + w * 16;
  const bool wave_live = slot0 < nslots;  // wave-uniform
  const int my_slot = min(slot0 + nn, nslots - 1);  // (the slot this lane's softmax state belongs to)
  const int my_lim = limit_of(my_slot);
  shalf8_t qf[NJ];
  {
    const int b = gr.first + (PHASE == 0 ? my_slot / g_full : member), head = ihkv * g_full + (PHASE == 0 ? my_slot % g_full : my_slot);
    const float* qr = p.q + (long long)b * p.step_q_bs + (long long)head * p.step_q_head_num + 8 * g;
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int i = 0; i < 8; i++) qf[j][i] = (_Float16)qr[32 * j + i];
  }
  sfloatx4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; dt++) o[dt] = sfloatx4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const float sc = p.qk_scale * 1.4426950408889634f;  // scores in the exp2 domain
  const int visible = min(range_end, my_lim);
  int vis_wave = range_end;  // what every live slot of the wave sees
  if constexpr (PHASE == 0) {
    int least = slot0 + nn < nslots ? my_lim : INT_MAX;
#pragma unroll
    for (int o2 = 8; o2 > 0; o2 >>= 1) least = min(least, __shfl_xor(least, o2, 64));
    vis_wave = min(range_end, __builtin_amdgcn_readfirstlane(least));
  }

  const int vp = (tid >> 3) * 2, vc = tid & 7;  // V^T staging: this thread's two neighbouring positions, its CH head dims
  shalf8_t kn[NT][NJ], vn[2][CH / 8];
  int ids[NT];
  const int* tab = sp.pg.table + (long long)table_row * sp.pg.table_stride;
  auto fetch_ids = [&](int pos0) {
#pragma unroll
    for (int t = 0; t < NT; t++) ids[t] = pos0 + 16 * t < kv_lim ? tab[(pos0 + 16 * t) >> sp.pg.block_shift] : -1;
  };
  auto fetch_k = [&](int pos0) {  // every address is attn_page_at's; its -1 is a load that is not issued and a register of zeros
    if (!wave_live) return;
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const long long cell = attn_page_at(sp.pg, ids[t], min(pos0 + 16 * t + nn, kv_lim - 1), p.step_k_sl);  // (the clamp stays inside the tile's page)
#pragma unroll
      for (int j = 0; j < NJ; j++) kn[t][j] = cell >= 0 ? *reinterpret_cast<const shalf8_t*>(kb + cell + 8 * g + 32 * j) : shalf8_t{0, 0, 0, 0, 0, 0, 0, 0};
    }
  };
  auto fetch_v = [&](int pos0) {
#pragma unroll
    for (int q2 = 0; q2 < 2; q2++) {
      const long long cell = attn_page_at(sp.pg, ids[vp >> 4], min(pos0 + vp + q2, kv_lim - 1), p.step_v_sl);
#pragma unroll
      for (int u = 0; u < CH / 8; u++) vn[q2][u] = cell >= 0 ? *reinterpret_cast<const shalf8_t*>(vb + cell + vc * CH + 8 * u) : shalf8_t{0, 0, 0, 0, 0, 0, 0, 0};
    }
  };
  fetch_ids(range_begin);
  fetch_k(range_begin);  // (range_begin < kv_lim: the range holds a key)
  fetch_v(range_begin);
  fetch_ids(range_begin + kBlkKB);
  for (int pos0 = range_begin; pos0 < range_end; pos0 += kBlkKB) {
    const bool more = pos0 + kBlkKB < range_end;
    shalf8_t pf[NH];  // slice h covers positions pos0 + 32 h ..: k-slot 8g + i <-> position 32 h + 16 (i >> 2) + 4g + (i & 3)
    float ar[4];
    if (wave_live) {
      sfloatx4 sv[NT];
#pragma unroll
      for (int t = 0; t < NT; t++) {
        sv[t] = sfloatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; j++) sv[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kn[t][j], qf[j], sv[t], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (more) fetch_k(pos0 + kBlkKB);
      __builtin_amdgcn_sched_barrier(0);
      float x[4 * NT], mx = -INFINITY;
      if (pos0 + kBlkKB <= vis_wave) {  // wave-uniform: every live slot of this wave sees the whole block
#pragma unroll
        for (int e = 0; e < 4 * NT; e++) {
          x[e] = sv[e >> 2][e & 3] * sc;
          mx = fmaxf(mx, x[e]);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4 * NT; e++) {
          const int pos = pos0 + 16 * (e >> 2) + 4 * g + (e & 3);
          x[e] = pos < visible ? sv[e >> 2][e & 3] * sc : -INFINITY;
          mx = fmaxf(mx, x[e]);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;  // nothing visible yet: every exp2 below is exp2(-inf) = 0
      const float alpha = exp2f(m_run - m_use);
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < 4 * NT; e++) {
        const float pe = exp2f(x[e] - m_use);
        ps += pe;
        pf[e >> 3][e & 7] = (_Float16)pe;
      }
      ps += __shfl_xor(ps, 16, 64);
      ps += __shfl_xor(ps, 32, 64);
      l_run = l_run * alpha + ps;
      m_run = m_new;
#pragma unroll
      for (int r = 0; r < 4; r++) ar[r] = __shfl(alpha, 4 * g + r, 64);
    }

    __syncthreads();  // the previous block's V^T reads are done
    {
      // V^T[d][pos] for the block: (pos, pos + 1) pairs as 4-byte LDS stores; positions at or behind the fetch limit hold zeros (P is zero there; keeps
      // 0 * x away from the inf / nan bits a pool may hold behind a live length)
      if (pos0 + kBlkKB <= kv_lim) {
#pragma unroll
        for (int i = 0; i < CH; i++)
          *reinterpret_cast<shalf2_t*>(vt + (vc * CH + i) * kBlkVStr + vp) = shalf2_t{vn[0][i >> 3][i & 7], vn[1][i >> 3][i & 7]};
      } else {
        const bool ok0 = pos0 + vp < kv_lim, ok1 = pos0 + vp + 1 < kv_lim;
#pragma unroll
        for (int i = 0; i < CH; i++) {
          const _Float16 a0 = ok0 ? vn[0][i >> 3][i & 7] : (_Float16)0.f, a1 = ok1 ? vn[1][i >> 3][i & 7] : (_Float16)0.f;
          *reinterpret_cast<shalf2_t*>(vt + (vc * CH + i) * kBlkVStr + vp) = shalf2_t{a0, a1};
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (more) fetch_v(pos0 + kBlkKB);
      fetch_ids(pos0 + 2 * kBlkKB);  // of the block the NEXT step requests
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    if (wave_live) {
#pragma unroll
      for (int dt = 0; dt < NDT; dt++) {
#pragma unroll
        for (int r = 0; r < 4; r++) o[dt][r] *= ar[r];
#pragma unroll
        for (int h = 0; h < NH; h++) {
          const _Float16* vr = vt + (16 * dt + nn) * kBlkVStr + 32 * h + 4 * g;
          const shalf4_t lo = *reinterpret_cast<const shalf4_t*>(vr), hi = *reinterpret_cast<const shalf4_t*>(vr + 16);
          const shalf8_t vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf[h], vf, o[dt], 0, 0, 0);
        }
      }
    }
  }
  if (!wave_live) return;
  // the record of slot slot0 + 4g + r: its (m, l) live in lane 4g + r; m leaves the exp2 domain (the merge forms expf(m_s - m))
  const float m_nat = m_run * 0.6931471805599453f;  // (-inf stays -inf)
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const float mr = __shfl(m_nat, 4 * g + r, 64), lr = __shfl(l_run, 4 * g + r, 64);
    const int slot = slot0 + 4 * g + r;
    if (slot >= nslots) continue;
    float* rec = record(slot);
    if (nn == 0) rec[0] = mr, rec[1] = lr;
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) rec[2 + 16 * dt + nn] = o[dt][r];
  }
}

// ============================================================================================================
// attn_shared_merge_kernel — one workgroup per (request, head): grid (heads, requests) x 128.  The request's group is found by a SCAN of dGroupStart
// (thread t looks at groups t, t + 128, ..; the lowest group that names the request wins), not through a request -> group map written by the prefix
// phase: a request that no group names must be left alone, so such a map would have to be cleared in front of every call — a fourth launch, or a
// memset node in the caller's graph — while the scan reads groups + 1 ints that the range launches have just brought into the cache.
// It reads the group's live prefix records, then the request's live suffix records (attn_block_live, as the range workgroups applied it), and sums
// attn_merge_kernel's sums in attn_merge_kernel's order (ns_attn_decode.hip: the weights expf(m_s - m), l and the accumulator columns summed over the
// records in ascending order), times out_scale, to dst and dst16.  l = 0 — an idle request, or one whose every table entry was unusable — gives zeros.
// ============================================================================================================
__global__ __launch_bounds__(128) void attn_shared_merge_kernel(const AttnSharedParams sp) {
  const AttnParams& p = sp.a;
  __shared__ int group_s;
  __shared__ float c_s[128];
  __shared__ float l_s[128];
  __shared__ float m_s[2];
  const int ihn = blockIdx.x, b = blockIdx.y;
  const int hs = p.head_size, t = threadIdx.x;
  if (t == 0) group_s = INT_MAX;
  __syncthreads();
  for (int g2 = t; g2 < sp.groups; g2 += 128) {
    const AttnSharedGroup cand = attn_shared_group(sp, g2);
    if (b >= cand.first && b < cand.first + cand.n) atomicMin(&group_s, g2);
  }
  __syncthreads();
  if (group_s == INT_MAX) return;  // no group names this request: its row is not touched (workgroup-uniform)
  const AttnSharedGroup gr = attn_shared_group(sp, group_s);
  const int len = attn_shared_len(sp, b);
  const int np = len > 0 ? attn_block_live(gr.prefix, sp.nsp, sp.kps_p, sp.min_keys).live : 0;
  const int ns = np + attn_block_live(len - gr.prefix, sp.nss, sp.kps_s, sp.min_keys).live;  // ns <= 128
  const float* wp = sp.ws + ((size_t)b * p.head_num + ihn) * sp.rec_stride * (2 + hs);
  auto at = [&](int s) { return wp + (size_t)(s < np ? s : sp.suf_off + s - np) * (2 + hs); };  // record s of the sum: prefix ranges, then suffix ranges
  float* dst = p.dst + (long long)b * p.step_dst_bs + (long long)ihn * p.step_dst_head_num;
  auto store = [&](int d, float ab, float lb) {
    const float y = lb > 0.f ? ab / lb * p.out_scale : 0.f;
    dst[d] = y;
    if (p.dst16) p.dst16[dst - p.dst + d] = (_Float16)y;
  };
  auto fast = [&](auto n_c) {  // (attn_merge_kernel's: every thread fetches all (max, sum) pairs and its own column in one batch of loads)
    constexpr int N = decltype(n_c)::value;
    float mv[N], lv[N], ov[N];
#pragma unroll
    for (int s2 = 0; s2 < N; s2++) {
      const bool on = s2 < ns;
      const float* r = at(on ? s2 : 0);
      mv[s2] = on ? r[0] : -INFINITY;
      lv[s2] = on ? r[1] : 0.f;
      ov[s2] = (on && t < hs) ? r[2 + t] : 0.f;
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
    if (t < hs) store(t, ab2, lb2);
  };
  if (ns <= 16) return fast(std::integral_constant<int, 16>{});  // (head sizes 64 and 128: one column per thread)
  if (ns <= 32) return fast(std::integral_constant<int, 32>{});
  float ms = -INFINITY, ls = 0.f;
  if (t < ns) {
    ms = at(t)[0];
    ls = at(t)[1];
  }
  float mb = ms;
#pragma unroll
  for (int o2 = 32; o2 > 0; o2 >>= 1) mb = fmaxf(mb, __shfl_xor(mb, o2, 64));
  if ((t & 63) == 0) m_s[t >> 6] = mb;
  __syncthreads();
  mb = fmaxf(m_s[0], m_s[1]);
  c_s[t] = (t < ns && ms != -INFINITY) ? expf(ms - mb) : 0.f;
  l_s[t] = ls;
  __syncthreads();
  float lb = 0.f;
  for (int s = 0; s < ns; s++) lb += l_s[s] * c_s[s];
  if (t < hs) {
    float ab = 0.f;
#pragma unroll 8
    for (int s = 0; s < ns; s++) ab += at(s)[2 + t] * c_s[s];
    store(t, ab, lb);
  }
}

// ---- launch of a plan (attn_shared_paged_plan); ws: pl.partial_bytes of device memory: three launches, one behind the other on st ------------------
hipError_t launch_attn_shared_paged(const AttnSharedPagedPlan& pl, float* ws, hipStream_t st) {
  AttnSharedParams sp = pl.sp;
  sp.ws = ws;
  if (pl.hs_pad == 64)
    hipLaunchKernelGGL((attn_shared_kernel<64, 0>), pl.grid_prefix, pl.block, 0, st, sp);
  else
    hipLaunchKernelGGL((attn_shared_kernel<128, 0>), pl.grid_prefix, pl.block, 0, st, sp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (pl.hs_pad == 64)
    hipLaunchKernelGGL((attn_shared_kernel<64, 1>), pl.grid_suffix, pl.block, 0, st, sp);
  else
    hipLaunchKernelGGL((attn_shared_kernel<128, 1>), pl.grid_suffix, pl.block, 0, st, sp);
  e = hipGetLastError();
  return e != hipSuccess ? e : launch_attn_shared_merge(sp, pl.merge_grid, st);
}
// the merge alone, over sp.ws: the partials do not know the cache's type (ns_attn_shared_f8.hip launches its own range kernels in front of it)
hipError_t launch_attn_shared_merge(const AttnSharedParams& sp, dim3 merge_grid, hipStream_t st) {
  hipLaunchKernelGGL(attn_shared_merge_kernel, merge_grid, dim3(128), 0, st, sp);
  return hipGetLastError();
}
void touch_attn_shared_module() { touch_kernel(reinterpret_cast<const void*>(attn_shared_kernel<128, 0>)); }

}  // namespace ns
