// ns_attn_block.hip — fused attention for a short block of query rows (2 .. 127) over a long cache: the 64-row matrix-core loop of
// attn_mfma_kernel (ns_attn_prefill.hip) over ONE RANGE of keys per workgroup, partial (m, l, acc) records per range, attn_merge_kernel
// (ns_attn_decode.hip) behind it.  Opt-in: ns_hip_set_tuning("attn_block_split", keys), AP_BLOCK_SPLIT of ns_attn_plan.cpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

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
// ============================================================================================================
typedef _Float16 bhalf8_t __attribute__((ext_vector_type(8)));
typedef _Float16 bhalf4_t __attribute__((ext_vector_type(4)));
typedef _Float16 bhalf2_t __attribute__((ext_vector_type(2)));
typedef float bfloatx4 __attribute__((ext_vector_type(4)));
constexpr int kBlkKB = 64;            // kv positions per block
constexpr int kBlkVStr = kBlkKB + 4;  // halves per V^T row in LDS: keeps the 8-byte reads aligned, skews banks

template <int HS>
__global__ __launch_bounds__(256) void attn_block_split_kernel(const AttnSplitParams sp) {
  constexpr int NJ = HS / 32, NDT = HS / 16, CH = HS / 8;  // k-slices of QK^T, output column tiles, V halves per thread
  constexpr int REC = 2 + HS;                              // floats per partial record
  __shared__ __attribute__((aligned(16))) _Float16 vt[HS * kBlkVStr];
  const AttnParams& p = sp.a;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, nn = l & 15, g = l >> 4;
  const int ihkv = int(blockIdx.x) % p.heads_kv, sblk = int(blockIdx.x) / p.heads_kv;  // neighbouring workgroups: neighbouring kv heads
  const int split = blockIdx.y, ibs = blockIdx.z;
  const int g_full = sp.g_full, nslots = p.sl_q * g_full;
  const bool causal = (p.flags & NS_ATTN_FLAG_IS_CAUSAL) != 0;
  const int off = p.sl_kv - p.sl_q;
  const int slot0 = sblk * 64 + w * 16;
  const int slot_last = min(sblk * 64 + 63, nslots - 1);  // the block's last live slot
  const int kv_end = causal ? min(p.sl_kv, slot_last / g_full + off + 1) : p.sl_kv;  // workgroup-uniform
  const int range_begin = split * sp.keys_per_split;
  const int range_end = min(range_begin + sp.keys_per_split, kv_end);
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
  const _Float16* kb = p.k + ibs * p.step_k_bs + ihkv * p.step_k_head_num;
  const _Float16* vb = p.v + ibs * p.step_v_bs + ihkv * p.step_v_head_num;

  const int my_slot = min(slot0 + nn, nslots - 1);  // (the slot this lane's softmax state belongs to)
  const int my_row = my_slot / g_full;
  bhalf8_t qf[NJ];
  {
    const float* qr = p.q + ibs * p.step_q_bs + (long long)(ihkv * g_full + my_slot % g_full) * p.step_q_head_num + (long long)my_row * p.step_q_sl + 8 * g;
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
  const int visible = min(range_end, causal ? my_row + off + 1 : p.sl_kv);                              // mha_dense_wrapper.h:1440-1441, within the range
  const int vis_wave = min(range_end, causal ? min(slot0, nslots - 1) / g_full + off + 1 : p.sl_kv);   // what the wave's FIRST slot sees

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
  auto fetch_k = [&](int pos0) {
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
  fetch_k(range_begin);  // (range_begin < kv_end <= sl_kv: the range holds a key)
  fetch_v(range_begin);
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
      if (pos0 + kBlkKB <= p.sl_kv) {
#pragma unroll
        for (int i = 0; i < CH; i++)
          *reinterpret_cast<bhalf2_t*>(vt + (vc * CH + i) * kBlkVStr + vp) = bhalf2_t{vn[0][i >> 3][i & 7], vn[1][i >> 3][i & 7]};
      } else {
        const bool ok0 = pos0 + vp < p.sl_kv, ok1 = pos0 + vp + 1 < p.sl_kv;
#pragma unroll
        for (int i = 0; i < CH; i++) {
          const _Float16 a0 = ok0 ? vn[0][i >> 3][i & 7] : (_Float16)0.f, a1 = ok1 ? vn[1][i >> 3][i & 7] : (_Float16)0.f;
          *reinterpret_cast<bhalf2_t*>(vt + (vc * CH + i) * kBlkVStr + vp) = bhalf2_t{a0, a1};
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (more) fetch_v(pos0 + kBlkKB);
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
void touch_attn_block_module() { touch_kernel(reinterpret_cast<const void*>(attn_block_split_kernel<128>)); }

}  // namespace ns
