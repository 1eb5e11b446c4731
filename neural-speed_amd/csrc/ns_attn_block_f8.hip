// ns_attn_block_f8.hip — ragged query blocks over an FP8 (E4M3) paged KV cache: the kernel of ns_hip_attn_block_paged_f8 and the launch of its plan
// (attn_block_paged_f8_plan, ns_attn_plan.cpp).  The pools are those of ns_hip_attn_decode_paged_f8 (ns_attn.h, "an FP8 paged cache"): one byte per
// element, every stride in bytes, one scale per pool, folded on the host into qk_scale / out_scale.  Q, the partials and the output are fp32 as ever,
// so attn_block_paged_merge_kernel (ns_attn_block.hip) serves unchanged.
//
// attn_block_split8_kernel<HS> is attn_block_split_kernel<HS, true> (ns_attn_block.hip, whose header describes the slots, the ranges, the partial
// records, the table ids fetched one block ahead and the exp2-domain softmax) with another K / V data path:
//   K   lane (key nn, group g) loads 16 BYTES per 64 dims of its key row — dims 64 j' + 16 g .. + 15, j' < HS / 64 — where the fp16 kernel loads 16
//       bytes per 32 dims: HS / 16 loads per lane and 64-key block instead of HS / 8.  The 16 codes decode to TWO operands of
//       v_mfma_f32_16x16x32_f16: the low 8 bytes are k-step 2 j', the high 8 bytes k-step 2 j' + 1.  A dot product does not care which k-slot holds
//       which dim as long as both operands agree, so the Q fragments are loaded to match: qf[2 j'][i] = q[64 j' + 16 g + i] and
//       qf[2 j' + 1][i] = q[64 j' + 16 g + 8 + i].  Nothing moves between lanes.
//   V   a thread's CH = HS / 8 dims of a position are CH bytes: one 16-byte load at head size 128, one 8-byte load at 64.  They are decoded once, at
//       staging, into the fp16 V^T image the fp16 kernel keeps in LDS (vt, kBlkVStr): a v_perm_b32 pairs the codes of the thread's two neighbouring
//       positions dim by dim, so that one packed conversion yields the (pos, pos + 1) pair of halves of one 4-byte LDS store.  P.V, its LDS reads and
//       the LDS footprint are the fp16 kernel's.
//   decode   E4M3 -> fp16 is exact (every E4M3 value is an fp16 value): v_cvt_scalef32_pk_f16_fp8 with scale 1.0, two codes per instruction.
// What lies behind a live length may be a NaN code: the row clamp to kv_len - 1 inside the tile's page, id -1 = no load and a register of zero CODES,
// scores selected rather than multiplied, and V's codes past kv_len selected to zero BEFORE they are decoded.  Every cell address is 64-bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "ns_attn.h"

namespace ns {

typedef _Float16 bhalf8_t __attribute__((ext_vector_type(8)));
typedef _Float16 bhalf4_t __attribute__((ext_vector_type(4)));
typedef _Float16 bhalf2_t __attribute__((ext_vector_type(2)));
typedef float bfloatx4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u4_t __attribute__((ext_vector_type(4)));

// eight E4M3 codes (two dwords, memory order) -> one MFMA operand of eight halves, exact
__device__ __forceinline__ bhalf8_t e4m3x8_to_h8(uint32_t w0, uint32_t w1) {
  const bhalf2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true);
  const bhalf2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true);
  return bhalf8_t{a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
}

template <int HS>
__global__ __launch_bounds__(256) void attn_block_split8_kernel(const AttnBlockPagedParams spp) {
  constexpr int NJ = HS / 32, NJ8 = HS / 64, NDT = HS / 16, CH = HS / 8;  // k-slices of QK^T, 16-byte K loads per key, output column tiles, V bytes per thread
  constexpr int REC = 2 + HS;                                             // floats per partial record
  typedef std::conditional_t<CH == 16, u4_t, u2_t> VCodes;               // a thread's CH codes of one position
  __shared__ __attribute__((aligned(16))) _Float16 vt[HS * kBlkVStr];
  const AttnSplitParams& sp = spp.sp;
  const AttnParams& p = sp.a;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, nn = l & 15, g = l >> 4;
  const int ihkv = int(blockIdx.x) % p.heads_kv, sblk = int(blockIdx.x) / p.heads_kv;  // neighbouring workgroups: neighbouring kv heads
  const int split = blockIdx.y, ibs = blockIdx.z;
  // the request's own geometry — its query rows, its live keys, the live ranges of that length (attn_block_live)
  const int q0 = spp.q_start[ibs], sl_q = attn_block_q_len(spp.q_start, ibs, p.sl_q), kv_len = attn_live_kv<true>(sp, ibs);
  if (sblk * 64 >= sl_q * sp.g_full) return;  // no slot of this block is a row of the request (workgroup-uniform, in front of any barrier)
  const AttnBlockLive lv = attn_block_live(kv_len, sp.nsplit, sp.keys_per_split, sp.dyn_min_keys);
  if (split >= lv.live) return;  // not a live range: the merge reads lv.live records
  const int kps = lv.kps;
  const int g_full = sp.g_full, nslots = sl_q * g_full;
  const bool causal = (p.flags & NS_ATTN_FLAG_IS_CAUSAL) != 0;
  const int off = kv_len - sl_q;
  const int slot0 = sblk * 64 + w * 16;
  const int slot_last = min(sblk * 64 + 63, nslots - 1);                        // the block's last live slot
  const int kv_end = causal ? min(kv_len, slot_last / g_full + off + 1) : kv_len;  // workgroup-uniform
  const int range_begin = split * kps;
  const int range_end = min(range_begin + kps, kv_end);
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
  const unsigned char* kb = reinterpret_cast<const unsigned char*>(p.k) + ihkv * p.step_k_head_num;  // the pools: bytes
  const unsigned char* vb = reinterpret_cast<const unsigned char*>(p.v) + ihkv * p.step_v_head_num;

  const int my_slot = min(slot0 + nn, nslots - 1);  // (the slot this lane's softmax state belongs to)
  const int my_row = my_slot / g_full;
  bhalf8_t qf[NJ];  // k-step 2 j': dims 64 j' + 16 g .. + 7, k-step 2 j' + 1: dims 64 j' + 16 g + 8 .. + 15 — the two halves of a 16-byte K load
  {
    const float* qr = p.q + (long long)(ihkv * g_full + my_slot % g_full) * p.step_q_head_num + (long long)(q0 + my_row) * p.step_q_sl + 16 * g;
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int i = 0; i < 8; i++) qf[j][i] = (_Float16)qr[64 * (j >> 1) + 8 * (j & 1) + i];
  }
  bfloatx4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; dt++) o[dt] = bfloatx4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const float sc = p.qk_scale * 1.4426950408889634f;  // scores in the exp2 domain
  const int visible = min(range_end, causal ? my_row + off + 1 : kv_len);
  const int vis_wave = min(range_end, causal ? min(slot0, nslots - 1) / g_full + off + 1 : kv_len);  // what the wave's FIRST slot sees

  constexpr int NT = kBlkKB / 16, NH = kBlkKB / 32;  // score tiles, 32-deep P.V slices per block
  const int vp = (tid >> 3) * 2, vc = tid & 7;        // V^T staging: this thread's two neighbouring positions, its CH head dims
  u4_t kn[NT][NJ8];  // the codes as loaded: half the fp16 kernel's staging registers
  VCodes vn[2];
  // Score tile t of a block (16 keys; also the 16 positions of V that wave t stages) lies in ONE page: ids[t], workgroup-uniform, -1 for a tile that
  // starts at or behind the live length — fetched a whole block ahead of the K / V requests it addresses.  Every address is attn_page_at's; its -1 is
  // a load that is not issued and a register of zero codes.
  int ids[NT];
  auto fetch_ids = [&](int pos0) {
    const int* tab = spp.pg.table + (long long)ibs * spp.pg.table_stride;
#pragma unroll
    for (int t = 0; t < NT; t++) ids[t] = pos0 + 16 * t < kv_len ? tab[(pos0 + 16 * t) >> spp.pg.block_shift] : -1;
  };
  auto fetch_k = [&](int pos0) {
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const long long cell = attn_page_at(spp.pg, ids[t], min(pos0 + 16 * t + nn, kv_len - 1), p.step_k_sl);  // (the clamp stays inside the tile's page)
#pragma unroll
      for (int j = 0; j < NJ8; j++) kn[t][j] = cell >= 0 ? *reinterpret_cast<const u4_t*>(kb + cell + 64 * j + 16 * g) : u4_t{0u, 0u, 0u, 0u};
    }
  };
  auto fetch_v = [&](int pos0) {
#pragma unroll
    for (int q2 = 0; q2 < 2; q2++) {
      const long long cell = attn_page_at(spp.pg, ids[vp >> 4], min(pos0 + vp + q2, kv_len - 1), p.step_v_sl);
      vn[q2] = cell >= 0 ? *reinterpret_cast<const VCodes*>(vb + cell + vc * CH) : VCodes(0u);
    }
  };
  fetch_ids(range_begin);
  fetch_k(range_begin);  // (range_begin < kv_end <= kv_len: the range holds a key)
  fetch_v(range_begin);
  fetch_ids(range_begin + kBlkKB);
  for (int pos0 = range_begin; pos0 < range_end; pos0 += kBlkKB) {
    const bool more = pos0 + kBlkKB < range_end;
    bfloatx4 sv[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {
      sv[t] = bfloatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NJ8; j++) {
        sv[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(e4m3x8_to_h8(kn[t][j].x, kn[t][j].y), qf[2 * j], sv[t], 0, 0, 0);
        sv[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(e4m3x8_to_h8(kn[t][j].z, kn[t][j].w), qf[2 * j + 1], sv[t], 0, 0, 0);
      }
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
      // V^T[d][pos] for the block: (pos, pos + 1) pairs as 4-byte LDS stores.  A position at or past kv_len holds zeros (P is zero there; the pool
      // holds anything behind the live length): its CODES are selected to zero, then decoded.  v_perm_b32 (selector bytes 0 .. 3: its second
      // operand, 4 .. 7: its first) pairs dim by dim: lo = (a0 b0 a1 b1), hi = (a2 b2 a3 b3) for the codes a of pos and b of pos + 1.
      const VCodes c0 = pos0 + vp < kv_len ? vn[0] : VCodes(0u), c1 = pos0 + vp + 1 < kv_len ? vn[1] : VCodes(0u);
#pragma unroll
      for (int wd = 0; wd < CH / 4; wd++) {
        const uint32_t lo = __builtin_amdgcn_perm(c1[wd], c0[wd], 0x05010400u), hi = __builtin_amdgcn_perm(c1[wd], c0[wd], 0x07030602u);
        _Float16* col = vt + (vc * CH + 4 * wd) * kBlkVStr + vp;
        *reinterpret_cast<bhalf2_t*>(col) = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false);
        *reinterpret_cast<bhalf2_t*>(col + kBlkVStr) = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true);
        *reinterpret_cast<bhalf2_t*>(col + 2 * kBlkVStr) = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false);
        *reinterpret_cast<bhalf2_t*>(col + 3 * kBlkVStr) = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (more) fetch_v(pos0 + kBlkKB);
      fetch_ids(pos0 + 2 * kBlkKB);  // of the block the NEXT step requests
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

// ---- launch of a plan (attn_block_paged_f8_plan); ws: pl.partial_bytes of device memory -------------------------------------------------------------
hipError_t launch_attn_block_paged_f8(const AttnBlockPagedPlan& pl, float* ws, hipStream_t st) {
  if (!pl.ok || !pl.f8) return hipErrorInvalidValue;
  AttnBlockPagedParams pp = pl.pp;
  pp.sp.ws = ws, pp.sp.tickets = nullptr;
  if (pl.hs_pad == 64)
    hipLaunchKernelGGL(attn_block_split8_kernel<64>, pl.grid, pl.block, 0, st, pp);
  else
    hipLaunchKernelGGL(attn_block_split8_kernel<128>, pl.grid, pl.block, 0, st, pp);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : launch_attn_block_paged_merge(pp, pl.merge_grid, st);  // the partials do not know the cache's type
}
void touch_attn_block_f8_module() { touch_kernel(reinterpret_cast<const void*>(attn_block_split8_kernel<128>)); }

}  // namespace ns
