// ns_attn_block.hip — fused attention for a short block of query rows (2 .. 127) over a long cache: the 64-row matrix-core loop of
// attn_mfma_kernel (ns_attn_prefill.hip) over ONE RANGE of keys per workgroup, partial (m, l, acc) records per range, attn_merge_kernel
// (ns_attn_decode.hip) behind it.  Opt-in: ns_hip_set_tuning("attn_block_split", keys), AP_BLOCK_SPLIT of ns_attn_plan.cpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "ns_attn.h"

namespace ns {

// ============================================================================================================
// attn_block_split_kernel — attn_mfma_kernel's loop (same MFMA operand layout, V^T staged through LDS, K / V requested one block ahead,
// exp2-domain online softmax; its header comment describes them, and the accumulator-row / softmax-row mismatch of the 16x16x32 layout) with
// three differences:
//   slots     A workgroup serves one KV head.  Its 64 row positions are slots: slot = row * g_full + j is query row `row` of query head
//             ihkv * g_full + j.  K / V of the kv head are read once for all query heads of its group (g_full = 1: plain rows).  Each lane derives
//             its Q row, its causal limit and the (row, head) it writes under from its slot; slots past sl_q * g_full load what the last live slot
//             loads and write nothing.  Slots are row-major, so the first slot of a wave has the wave's smallest causal limit: the wave-uniform
//             "whole block visible" test stays on it.
//   a range   blockIdx.y = split walks keys [split * kps, min((split + 1) * kps, kv_end)) in 64-key blocks (kps a multiple of 64); kv_end = the
//             causal limit of the block's last live slot.  Scores are masked at min(visible, range end); the fetch clamps and the zero fill of V^T
//             stay tied to sl_kv (a library-managed cache has NaN bytes behind its rows).
//   partials  no division by l, no out_scale: every live slot writes (m in natural-log units, l, acc[hs]) at
//             ws[batch][row][head][split][2 + hs]; a slot that saw no key writes (-inf, 0, zeros), which the merge weighs 0.  A workgroup
//             whose range starts at or past kv_end writes that for all its live slots and leaves before any barrier (workgroup-uniform).
// grid (slot_blocks * heads_kv, nsplit, batch), 256 threads; wave w owns slots 16w .. 16w + 15 of the block.
// PAGED (ns_hip_attn_block_paged; argument block AttnBlockPagedParams, ns_attn.h): ragged query blocks over a paged cache.  blockIdx.z is a REQUEST
// with its own number of query rows (packed rows q_start[b] ..) and its own live keys (kmove[b] + kdelta), over which the workgroups apply the range
// rule themselves (attn_block_live); K / V come from the pools through the block table.  The uniform instantiations hold the instructions they held
// without it (docs/kernels/attention.md, "Ragged query blocks over a paged cache").
// ============================================================================================================
typedef _Float16 bhalf8_t __attribute__((ext_vector_type(8)));
typedef _Float16 bhalf4_t __attribute__((ext_vector_type(4)));
typedef _Float16 bhalf2_t __attribute__((ext_vector_type(2)));
typedef float bfloatx4 __attribute__((ext_vector_type(4)));
constexpr int kBlkKB = 64;            // kv positions per block
constexpr int kBlkVStr = kBlkKB + 4;  // halves per V^T row in LDS: keeps the 8-byte reads aligned, skews banks

__device__ __forceinline__ const AttnSplitParams& split_params(const AttnSplitParams& sp) { return sp; }
__device__ __forceinline__ const AttnSplitParams& split_params(const AttnBlockPagedParams& pp) { return pp.sp; }

template <int HS, bool PAGED = false>
__global__ __launch_bounds__(256) void attn_block_split_kernel(const std::conditional_t<PAGED, AttnBlockPagedParams, AttnSplitParams> spp) {
  constexpr int NJ = HS / 32, NDT = HS / 16, CH = HS / 8;  // k-slices of QK^T, output column tiles, V halves per thread
  constexpr int REC = 2 + HS;                              // floats per partial record
  __shared__ __attribute__((aligned(16))) _Float16 vt[HS * kBlkVStr];
  const AttnSplitParams& sp = split_params(spp);
  const AttnParams& p = sp.a;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, nn = l & 15, g = l >> 4;
  const int ihkv = int(blockIdx.x) % p.heads_kv, sblk = int(blockIdx.x) / p.heads_kv;  // neighbouring workgroups: neighbouring kv heads
  const int split = blockIdx.y, ibs = blockIdx.z;
  // PAGED: the request's own geometry — its query rows, its live keys, the live ranges of that length (attn_block_live)
  int q0 = 0, q_len = 0, kv_len = 0, kps_live = 0;
  if constexpr (PAGED) {
    q0 = spp.q_start[ibs];
    q_len = attn_block_q_len(spp.q_start, ibs, p.sl_q);
    kv_len = attn_live_kv<true>(sp, ibs);
    if (sblk * 64 >= q_len * sp.g_full) return;  // no slot of this block is a row of the request (workgroup-uniform, in front of any barrier)
    const AttnBlockLive lv = attn_block_live(kv_len, sp.nsplit, sp.keys_per_split, sp.dyn_min_keys);
    if (split >= lv.live) return;  // not a live range: the merge reads lv.live records
    kps_live = lv.kps;
  }
  // (read where they are used, so that the uniform instantiations hold the instructions they held without the PAGED ones)
  auto sl_q = [&] { if constexpr (PAGED) return q_len; else return p.sl_q; };
  auto sl_kv = [&] { if constexpr (PAGED) return kv_len; else return p.sl_kv; };
  auto kps = [&] { if constexpr (PAGED) return kps_live; else return sp.keys_per_split; };
  const int g_full = sp.g_full, nslots = sl_q() * g_full;
  const bool causal = (p.flags & NS_ATTN_FLAG_IS_CAUSAL) != 0;
  const int off = sl_kv() - sl_q();
  const int slot0 = sblk * 64 + w * 16;
  const int slot_last = min(sblk * 64 + 63, nslots - 1);  // the block's last live slot
  const int kv_end = causal ? min(sl_kv(), slot_last / g_full + off + 1) : sl_kv();  // workgroup-uniform
  const int range_begin = split * kps();
  const int range_end = min(range_begin + kps(), kv_end);
  float* wsb = sp.ws + (size_t)ibs * p.sl_q * p.head_num * sp.nsplit * REC;
  auto record = [&](int slot) {  // of a live slot, for this range
    const int row = slot / g_full, head = ihkv * g_full + slot % g_full;
    return wsb + (((size_t)row * p.head_num + head) * sp.nsplit + split) * REC;
  };
  if (range_begin >= kv_end) {  // no slot of this block sees a key of this range: the merge still reads every record
    for (int e = tid; e < 64 * REC; e += 256) {
      const int slot = sblk * 64 + e / REC, c = e % REC;
      if (slot < nslots) record(slot)[c] = c == 0 ? -INFINITY : 0.f;
    }
    return;
  }
  const _Float16* kb = p.k + ibs * p.step_k_bs + ihkv * p.step_k_head_num;  // (PAGED: the pools — the plan's step_k_bs / step_v_bs are 0)
  const _Float16* vb = p.v + ibs * p.step_v_bs + ihkv * p.step_v_head_num;

  const int my_slot = min(slot0 + nn, nslots - 1);  // (the slot this lane's softmax state belongs to)
  const int my_row = my_slot / g_full;
  bhalf8_t qf[NJ];
  {
    const float* qr = p.q + ibs * p.step_q_bs + (long long)(ihkv * g_full + my_slot % g_full) * p.step_q_head_num + (long long)my_row * p.step_q_sl + 8 * g;
    if constexpr (PAGED) qr += (long long)q0 * p.step_q_sl;  // packed rows (the plan's step_q_bs is 0)
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int i = 0; i < 8; i++) qf[j][i] = (_Float16)qr[32 * j + i];
  }
  bfloatx4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; dt++) o[dt] = bfloatx4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const float sc = p.qk_scale * 1.4426950408889634f;  // scores in the exp2 domain
  const int visible = min(range_end, causal ? my_row + off + 1 : sl_kv());                              // mha_dense_wrapper.h:1440-1441, within the range
  const int vis_wave = min(range_end, causal ? min(slot0, nslots - 1) / g_full + off + 1 : sl_kv());   // what the wave's FIRST slot sees

  constexpr int NT = kBlkKB / 16, NH = kBlkKB / 32;  // score tiles, 32-deep P.V slices per block
  const int vp = (tid >> 3) * 2, vc = tid & 7;        // V^T staging: this thread's two neighbouring positions, its CH head dims
  bhalf8_t kn[NT][NJ], vn[2][CH / 8];
  const long long kstep_blk = (long long)kBlkKB * p.step_k_sl, vstep_blk = (long long)kBlkKB * p.step_v_sl;
  const _Float16* kp[NT];
  const _Float16* vpp[2];
#pragma unroll
  for (int t = 0; t < NT; t++) kp[t] = kb + (long long)(range_begin + 16 * t + nn) * p.step_k_sl + 8 * g;
#pragma unroll
  for (int q2 = 0; q2 < 2; q2++) vpp[q2] = vb + (long long)(range_begin + vp + q2) * p.step_v_sl + vc * CH;
  // PAGED: a block starts at a multiple of 64 and a page holds 16 keys or more, so score tile t of a block (16 keys; also the 16 positions of V that
  // wave t stages) lies in ONE page: ids[t], workgroup-uniform, -1 for a tile that starts at or behind the live length (whose table entry may hold
  // anything) — fetched a whole block ahead of the K / V requests it addresses (fetch_ids), not in front of them.  Every address is attn_page_at's;
  // its -1 (an id that is no block of the pool) is a load that is not issued and a register of zeros.
  int ids[NT];
  auto fetch_ids = [&](int pos0) {
    if constexpr (PAGED) {
      const int* tab = spp.pg.table + (long long)ibs * spp.pg.table_stride;
#pragma unroll
      for (int t = 0; t < NT; t++) ids[t] = pos0 + 16 * t < kv_len ? tab[(pos0 + 16 * t) >> spp.pg.block_shift] : -1;
    }
  };
  auto fetch_k_paged = [&](int pos0) {
    if constexpr (PAGED) {
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const long long cell = attn_page_at(spp.pg, ids[t], min(pos0 + 16 * t + nn, kv_len - 1), p.step_k_sl);  // (the clamp stays inside the tile's page)
#pragma unroll
        for (int j = 0; j < NJ; j++)
          kn[t][j] = cell >= 0 ? *reinterpret_cast<const bhalf8_t*>(kb + cell + 8 * g + 32 * j) : bhalf8_t{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  };
  auto fetch_v_paged = [&](int pos0) {
    if constexpr (PAGED) {
#pragma unroll
      for (int q2 = 0; q2 < 2; q2++) {
        const long long cell = attn_page_at(spp.pg, ids[vp >> 4], min(pos0 + vp + q2, kv_len - 1), p.step_v_sl);
#pragma unroll
        for (int u = 0; u < CH / 8; u++)
          vn[q2][u] = cell >= 0 ? *reinterpret_cast<const bhalf8_t*>(vb + cell + vc * CH + 8 * u) : bhalf8_t{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  };
  auto fetch_k = [&](int pos0) {
    if constexpr (PAGED) return fetch_k_paged(pos0);
    if (pos0 + kBlkKB <= p.sl_kv) {  // workgroup-uniform
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int j = 0; j < NJ; j++) kn[t][j] = *reinterpret_cast<const bhalf8_t*>(kp[t] + 32 * j);
    } else {
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const _Float16* kr = kb + (long long)min(pos0 + 16 * t + nn, p.sl_kv - 1) * p.step_k_sl + 8 * g;
#pragma unroll
        for (int j = 0; j < NJ; j++) kn[t][j] = *reinterpret_cast<const bhalf8_t*>(kr + 32 * j);
      }
    }
#pragma unroll
    for (int t = 0; t < NT; t++) kp[t] += kstep_blk;
  };
  auto fetch_v = [&](int pos0) {
    if constexpr (PAGED) return fetch_v_paged(pos0);
    if (pos0 + kBlkKB <= p.sl_kv) {
#pragma unroll
      for (int q2 = 0; q2 < 2; q2++)
#pragma unroll
        for (int u = 0; u < CH / 8; u++) vn[q2][u] = *reinterpret_cast<const bhalf8_t*>(vpp[q2] + 8 * u);
    } else {
#pragma unroll
      for (int q2 = 0; q2 < 2; q2++) {
        const _Float16* vr = vb + (long long)min(pos0 + vp + q2, p.sl_kv - 1) * p.step_v_sl + vc * CH;
#pragma unroll
        for (int u = 0; u < CH / 8; u++) vn[q2][u] = *reinterpret_cast<const bhalf8_t*>(vr + 8 * u);
      }
    }
#pragma unroll
    for (int q2 = 0; q2 < 2; q2++) vpp[q2] += vstep_blk;
  };
  fetch_ids(range_begin);
  fetch_k(range_begin);  // (range_begin < kv_end <= sl_kv: the range holds a key)
  fetch_v(range_begin);
  fetch_ids(range_begin + kBlkKB);
  for (int pos0 = range_begin; pos0 < range_end; pos0 += kBlkKB) {
    const bool more = pos0 + kBlkKB < range_end;
    bfloatx4 sv[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {
      sv[t] = bfloatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NJ; j++) sv[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kn[t][j], qf[j], sv[t], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (more) fetch_k(pos0 + kBlkKB);
    __builtin_amdgcn_sched_barrier(0);
    float x[4 * NT], mx = -INFINITY;
    if (pos0 + kBlkKB <= vis_wave) {  // wave-uniform: every slot of this wave sees the whole block
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
    bhalf8_t pf[NH];  // slice h covers positions pos0 + 32 h ..: k-slot 8g + i <-> position 32 h + 16 (i >> 2) + 4g + (i & 3)
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
    float ar[4];
#pragma unroll
    for (int r = 0; r < 4; r++) ar[r] = __shfl(alpha, 4 * g + r, 64);

    __syncthreads();  // the previous block's V^T reads are done
    {
      // V^T[d][pos] for the block: (pos, pos + 1) pairs as 4-byte LDS stores; positions past the end hold zeros (P is zero
      // there; keeps 0 * x away from inf / nan bits)
      // (PAGED: tied to the request's live length — the pool holds anything behind it; the fields named here, not through sl_kv(): that form
      // moves instructions of the uniform head-size-128 instantiation)
      if (pos0 + kBlkKB <= (PAGED ? kv_len : p.sl_kv)) {
#pragma unroll
        for (int i = 0; i < CH; i++)
          *reinterpret_cast<bhalf2_t*>(vt + (vc * CH + i) * kBlkVStr + vp) = bhalf2_t{vn[0][i >> 3][i & 7], vn[1][i >> 3][i & 7]};
      } else {
        const bool ok0 = pos0 + vp < (PAGED ? kv_len : p.sl_kv), ok1 = pos0 + vp + 1 < (PAGED ? kv_len : p.sl_kv);
#pragma unroll
        for (int i = 0; i < CH; i++) {
          const _Float16 a0 = ok0 ? vn[0][i >> 3][i & 7] : (_Float16)0.f, a1 = ok1 ? vn[1][i >> 3][i & 7] : (_Float16)0.f;
          *reinterpret_cast<bhalf2_t*>(vt + (vc * CH + i) * kBlkVStr + vp) = bhalf2_t{a0, a1};
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (more) fetch_v(pos0 + kBlkKB);
      if constexpr (PAGED) fetch_ids(pos0 + 2 * kBlkKB);  // of the block the NEXT step requests
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) {
#pragma unroll
      for (int r = 0; r < 4; r++) o[dt][r] *= ar[r];
#pragma unroll
      for (int h = 0; h < NH; h++) {
        const _Float16* vr = vt + (16 * dt + nn) * kBlkVStr + 32 * h + 4 * g;
        const bhalf4_t lo = *reinterpret_cast<const bhalf4_t*>(vr), hi = *reinterpret_cast<const bhalf4_t*>(vr + 16);
        const bhalf8_t vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf[h], vf, o[dt], 0, 0, 0);
      }
    }
  }
  // the record of slot slot0 + 4g + r: its (m, l) live in lane 4g + r; m leaves the exp2 domain (attn_merge_kernel forms expf(m_s - m))
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

// ---- launch of a plan (ns_attn_plan.cpp): pl.hs_pad is the template argument; ws: pl.partial_bytes of device memory ------------------------
hipError_t launch_attn_block_split(const AttnPlan& pl, float* ws, hipStream_t st) {
  AttnSplitParams sp = pl.sp;
  sp.ws = ws, sp.tickets = nullptr, sp.kmove = nullptr;  // (no merge inside the launch, no moving length)
  if (pl.hs_pad == 64)
    hipLaunchKernelGGL(attn_block_split_kernel<64>, pl.grid, pl.block, 0, st, sp);
  else
    hipLaunchKernelGGL(attn_block_split_kernel<128>, pl.grid, pl.block, 0, st, sp);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : launch_attn_merge(sp, pl.grid.z, st);
}

// ---- ns_hip_attn_block_paged -------------------------------------------------------------------------------------------------------------------------
// The merge behind the PAGED instantiation: attn_merge_kernel's sums in attn_merge_kernel's order (ns_attn_decode.hip: the weights expf(m_s - m), l and
// the accumulator columns summed over the ranges in ascending order), over the request's LIVE ranges (attn_block_live, as the range workgroups
// applied it), written to the request's packed row.  A row no range saw a key for — or that has no live range at all: a request without keys — has
// l = 0 and is written as zeros.  grid (heads, max_q, requests) x 128; the workgroups of rows the request does not have leave at once.
__global__ __launch_bounds__(128) void attn_block_paged_merge_kernel(const AttnBlockPagedParams pp) {
  const AttnSplitParams& sp = pp.sp;
  const AttnParams& p = sp.a;
  __shared__ float c_s[64];
  __shared__ float l_s[64];
  const int ihn = blockIdx.x, i = blockIdx.y, ibs = blockIdx.z;
  const int hs = p.head_size, t = threadIdx.x;
  if (i >= attn_block_q_len(pp.q_start, ibs, p.sl_q)) return;
  const int ns = attn_block_live(attn_live_kv<true>(sp, ibs), sp.nsplit, sp.keys_per_split, sp.dyn_min_keys).live;  // ns <= 64
  const float* wp = sp.ws + (((size_t)ibs * p.sl_q + i) * p.head_num + ihn) * sp.nsplit * (2 + hs);
  float* dst = p.dst + ihn * p.step_dst_head_num + (long long)(pp.q_start[ibs] + i) * p.step_dst_sl;
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
    if (t < hs) store(t, ab2, lb2);
  };
  if (ns <= 16) return fast(std::integral_constant<int, 16>{});  // (head sizes 64 and 128: one column per thread)
  if (ns <= 32) return fast(std::integral_constant<int, 32>{});
  float ms = -INFINITY, ls = 0.f;
  if (t < ns) {
    ms = wp[t * (2 + hs)];
    ls = wp[t * (2 + hs) + 1];
  }
  float mb = ms;
#pragma unroll
  for (int o2 = 32; o2 > 0; o2 >>= 1) mb = fmaxf(mb, __shfl_xor(mb, o2, 64));  // the ranges live in wave 0 (ns <= 64)
  if (t < 64) {
    c_s[t] = (t < ns && ms != -INFINITY) ? expf(ms - mb) : 0.f;
    l_s[t] = ls;
  }
  __syncthreads();
  float lb = 0.f;
  for (int s = 0; s < ns; s++) lb += l_s[s] * c_s[s];
  if (t < hs) {
    float ab = 0.f;
#pragma unroll 8
    for (int s = 0; s < ns; s++) ab += wp[s * (2 + hs) + 2 + t] * c_s[s];
    store(t, ab, lb);
  }
}

hipError_t launch_attn_block_paged(const AttnBlockPagedPlan& pl, float* ws, hipStream_t st) {
  AttnBlockPagedParams pp = pl.pp;
  pp.sp.ws = ws, pp.sp.tickets = nullptr;
  if (pl.hs_pad == 64)
    hipLaunchKernelGGL((attn_block_split_kernel<64, true>), pl.grid, pl.block, 0, st, pp);
  else
    hipLaunchKernelGGL((attn_block_split_kernel<128, true>), pl.grid, pl.block, 0, st, pp);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(attn_block_paged_merge_kernel, pl.merge_grid, dim3(128), 0, st, pp);
  return hipGetLastError();
}
void touch_attn_block_module() { touch_kernel(reinterpret_cast<const void*>(attn_block_split_kernel<128>)); }

}  // namespace ns
