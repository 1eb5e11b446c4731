// ns_attn_shared_f8.hip — shared-prefix (cascade) decode over an FP8 (E4M3) paged KV cache: the range kernels of ns_hip_attn_decode_paged_shared_f8 and
// the launch of its plan (attn_shared_paged_f8_plan, ns_attn_plan.cpp; argument block AttnSharedParams, ns_attn.h).  The pools are those of
// ns_hip_attn_decode_paged_f8 (ns_attn.h, "an FP8 paged cache"): one byte per element, every stride in bytes, one scale per pool, folded on the host
// into qk_scale / out_scale.  Q, the partial records and the output are fp32 as ever, so attn_shared_merge_kernel (ns_attn_shared.hip) serves unchanged.
//
// attn_shared8_kernel<HS, PHASE> has the GEOMETRY of attn_shared_kernel<HS, PHASE> (ns_attn_shared.hip, whose header describes it: slots as (member,
// head), the per-slot key limit min(P_g, len_b), the slot block's largest limit that ties the fetch clamp and the zero fill, the leader's table row in
// the prefix phase and the member's own in the suffix phase, idle waves, the early exits, the (-inf, 0, zeros) records) and the K / V DATA PATH of
// attn_block_split8_kernel<HS> (ns_attn_block_f8.hip):
//   K   lane (key nn, group g) loads 16 BYTES per 64 dims of its key row — dims 64 j' + 16 g .. + 15, j' < HS / 64.  The 16 codes decode in registers
//       to TWO operands of v_mfma_f32_16x16x32_f16: the low 8 bytes are k-step 2 j', the high 8 bytes k-step 2 j' + 1, and the Q fragments are loaded
//       to match: qf[2 j'][i] = q[64 j' + 16 g + i], qf[2 j' + 1][i] = q[64 j' + 16 g + 8 + i].  Nothing moves between lanes; the staging registers
//       hold codes, half of the fp16 kernel's kn.
//   V   a thread's CH = HS / 8 dims of a position are CH bytes: one 16-byte load at head size 128, one 8-byte load at 64.  A v_perm_b32 pairs the codes
//       of the thread's two neighbouring positions dim by dim, one packed conversion yields the (pos, pos + 1) pair of halves of one 4-byte LDS store
//       into the fp16 V^T image (vt, kBlkVStr) the fp16 kernel keeps.  P.V, its LDS reads and the LDS footprint are the fp16 kernel's.
//   decode   E4M3 -> fp16 is exact: v_cvt_scalef32_pk_f16_fp8 with scale 1.0, two codes per instruction.
// What lies at or behind the slot block's largest limit kv_lim (suffix phase: len_b) may be a NaN code (0x7f): the K row is clamped to kv_lim - 1 inside
// the tile's page, id -1 is a load that is not issued and a register of zero CODES, V's codes at or behind kv_lim are selected to zero BEFORE they are
// decoded, and scores are selected, not multiplied.  In the prefix phase the cells between a slot's own limit and kv_lim are another member's live
// keys — finite — and the per-slot score mask alone keeps them out of that slot's record.  Every cell address is attn_page_at's, with byte strides, 64-bit.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "ns_attn.h"

namespace ns {

typedef _Float16 chalf8_t __attribute__((ext_vector_type(8)));
typedef _Float16 chalf4_t __attribute__((ext_vector_type(4)));
typedef _Float16 chalf2_t __attribute__((ext_vector_type(2)));
typedef float cfloatx4 __attribute__((ext_vector_type(4)));
typedef uint32_t cu2_t __attribute__((ext_vector_type(2)));
typedef uint32_t cu4_t __attribute__((ext_vector_type(4)));

// eight E4M3 codes (two dwords, memory order) -> one MFMA operand of eight halves, exact
__device__ __forceinline__ chalf8_t shared8_e4m3x8_to_h8(uint32_t w0, uint32_t w1) {
  const chalf2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true);
  const chalf2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true);
  return chalf8_t{a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
}

// 256 threads; wave w owns slots 16w .. 16w + 15 of the block.  Ranges start at multiples of 16 (ns_attn.h), so score tile t of a block (16 keys; also
// the 16 positions of V that wave t stages) lies in ONE page: ids[t], workgroup-uniform, -1 for a tile that starts at or behind the fetch limit.
template <int HS, int PHASE>
__global__ __launch_bounds__(256) void attn_shared8_kernel(const AttnSharedParams sp) {
  constexpr int NJ = HS / 32, NJ8 = HS / 64, NDT = HS / 16, CH = HS / 8;  // k-slices of QK^T, 16-byte K loads per key, output column tiles, V bytes per thread
  constexpr int REC = 2 + HS;                                             // floats per partial record
  constexpr int NT = kBlkKB / 16, NH = kBlkKB / 32;                       // score tiles, 32-deep P.V slices per block
  typedef std::conditional_t<CH == 16, cu4_t, cu2_t> VCodes;             // a thread's CH codes of one position
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
  const unsigned char* kb = reinterpret_cast<const unsigned char*>(p.k) + ihkv * p.step_k_head_num;  // the pools: bytes
  const unsigned char* vb = reinterpret_cast<const unsigned char*>(p.v) + ihkv * p.step_v_head_num;
  const int slot0 = sblk * 64 + w * 16;
  const bool wave_live = slot0 < nslots;  // wave-uniform
  const int my_slot = min(slot0 + nn, nslots - 1);  // (the slot this lane's softmax state belongs to)
  const int my_lim = limit_of(my_slot);
  chalf8_t qf[NJ];  // k-step 2 j': dims 64 j' + 16 g .. + 7, k-step 2 j' + 1: dims 64 j' + 16 g + 8 .. + 15 — the two halves of a 16-byte K load
  {
    const int b = gr.first + (PHASE == 0 ? my_slot / g_full : member), head = ihkv * g_full + (PHASE == 0 ? my_slot % g_full : my_slot);
    const float* qr = p.q + (long long)b * p.step_q_bs + (long long)head * p.step_q_head_num + 16 * g;
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int i = 0; i < 8; i++) qf[j][i] = (_Float16)qr[64 * (j >> 1) + 8 * (j & 1) + i];
  }
  cfloatx4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; dt++) o[dt] = cfloatx4{0.f, 0.f, 0.f, 0.f};
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
  cu4_t kn[NT][NJ8];  // the codes as loaded
  VCodes vn[2];
  int ids[NT];
  const int* tab = sp.pg.table + (long long)table_row * sp.pg.table_stride;
  auto fetch_ids = [&](int pos0) {
#pragma unroll
    for (int t = 0; t < NT; t++) ids[t] = pos0 + 16 * t < kv_lim ? tab[(pos0 + 16 * t) >> sp.pg.block_shift] : -1;
  };
  auto fetch_k = [&](int pos0) {  // every address is attn_page_at's; its -1 is a load that is not issued and a register of zero codes
    if (!wave_live) return;
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const long long cell = attn_page_at(sp.pg, ids[t], min(pos0 + 16 * t + nn, kv_lim - 1), p.step_k_sl);  // (the clamp stays inside the tile's page)
#pragma unroll
      for (int j = 0; j < NJ8; j++) kn[t][j] = cell >= 0 ? *reinterpret_cast<const cu4_t*>(kb + cell + 64 * j + 16 * g) : cu4_t{0u, 0u, 0u, 0u};
    }
  };
  auto fetch_v = [&](int pos0) {
#pragma unroll
    for (int q2 = 0; q2 < 2; q2++) {
      const long long cell = attn_page_at(sp.pg, ids[vp >> 4], min(pos0 + vp + q2, kv_lim - 1), p.step_v_sl);
      vn[q2] = cell >= 0 ? *reinterpret_cast<const VCodes*>(vb + cell + vc * CH) : VCodes(0u);
    }
  };
  fetch_ids(range_begin);
  fetch_k(range_begin);  // (range_begin < kv_lim: the range holds a key)
  fetch_v(range_begin);
  fetch_ids(range_begin + kBlkKB);
  for (int pos0 = range_begin; pos0 < range_end; pos0 += kBlkKB) {
    const bool more = pos0 + kBlkKB < range_end;
    chalf8_t pf[NH];  // slice h covers positions pos0 + 32 h ..: k-slot 8g + i <-> position 32 h + 16 (i >> 2) + 4g + (i & 3)
    float ar[4];
    if (wave_live) {
      cfloatx4 sv[NT];
#pragma unroll
      for (int t = 0; t < NT; t++) {
        sv[t] = cfloatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ8; j++) {
          sv[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(shared8_e4m3x8_to_h8(kn[t][j].x, kn[t][j].y), qf[2 * j], sv[t], 0, 0, 0);
          sv[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(shared8_e4m3x8_to_h8(kn[t][j].z, kn[t][j].w), qf[2 * j + 1], sv[t], 0, 0, 0);
        }
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
      // V^T[d][pos] for the block: (pos, pos + 1) pairs as 4-byte LDS stores.  A position at or behind the fetch limit holds zeros (P is zero there;
      // the pool may hold NaN codes there): its CODES are selected to zero, then decoded.  v_perm_b32 (selector bytes 0 .. 3: its second operand,
      // 4 .. 7: its first) pairs dim by dim: lo = (a0 b0 a1 b1), hi = (a2 b2 a3 b3) for the codes a of pos and b of pos + 1.
      const VCodes c0 = pos0 + vp < kv_lim ? vn[0] : VCodes(0u), c1 = pos0 + vp + 1 < kv_lim ? vn[1] : VCodes(0u);
#pragma unroll
      for (int wd = 0; wd < CH / 4; wd++) {
        const uint32_t lo = __builtin_amdgcn_perm(c1[wd], c0[wd], 0x05010400u), hi = __builtin_amdgcn_perm(c1[wd], c0[wd], 0x07030602u);
        _Float16* col = vt + (vc * CH + 4 * wd) * kBlkVStr + vp;
        *reinterpret_cast<chalf2_t*>(col) = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false);
        *reinterpret_cast<chalf2_t*>(col + kBlkVStr) = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true);
        *reinterpret_cast<chalf2_t*>(col + 2 * kBlkVStr) = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false);
        *reinterpret_cast<chalf2_t*>(col + 3 * kBlkVStr) = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true);
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
          const chalf4_t lo = *reinterpret_cast<const chalf4_t*>(vr), hi = *reinterpret_cast<const chalf4_t*>(vr + 16);
          const chalf8_t vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
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

// ---- launch of a plan (attn_shared_paged_f8_plan); ws: pl.partial_bytes of device memory: three launches, one behind the other on st -----------------
hipError_t launch_attn_shared_paged_f8(const AttnSharedPagedPlan& pl, float* ws, hipStream_t st) {
  if (!pl.ok || !pl.f8) return hipErrorInvalidValue;
  AttnSharedParams sp = pl.sp;
  sp.ws = ws;
  if (pl.hs_pad == 64)
    hipLaunchKernelGGL((attn_shared8_kernel<64, 0>), pl.grid_prefix, pl.block, 0, st, sp);
  else
    hipLaunchKernelGGL((attn_shared8_kernel<128, 0>), pl.grid_prefix, pl.block, 0, st, sp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (pl.hs_pad == 64)
    hipLaunchKernelGGL((attn_shared8_kernel<64, 1>), pl.grid_suffix, pl.block, 0, st, sp);
  else
    hipLaunchKernelGGL((attn_shared8_kernel<128, 1>), pl.grid_suffix, pl.block, 0, st, sp);
  e = hipGetLastError();
  return e != hipSuccess ? e : launch_attn_shared_merge(sp, pl.merge_grid, st);  // the partials do not know the cache's type
}
void touch_attn_shared_f8_module() { touch_kernel(reinterpret_cast<const void*>(attn_shared8_kernel<128, 0>)); }

}  // namespace ns
