// ns_attn_prefill.hip — fused attention, the matrix-core kernels for 16 or more query rows (attn_mfma_kernel: 64 rows per workgroup;
// attn_mfma2_kernel, attn_mfma3_kernel: 128; attn_mfma2_paged_kernel: attn_mfma2_kernel's body over a paged cache, ns_hip_attn_prefill_paged), and the
// launch of a plan that names one (ns_attn.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "ns_attn.h"
#include "ns_launch.h"

namespace ns {

// ============================================================================================================
// attn_mfma_kernel — prefill / multi-row attention on the matrix cores (head size 64 or 128, contiguous head dim)
//
// One 256-thread workgroup = 64 query rows of one (batch, head); wave w owns rows 16w .. 16w+15.  KV positions are
// walked in blocks of 64 (four score tiles, two 32-deep P.V slices) with the online-softmax recurrence:
//   S^T = K . Q^T   v_mfma_f32_16x16x32_f16 with A = K rows (lane (nn, g): 16 B of K[pos0 + 16t + nn][32j + 8g ..]) and
//                   B = Q rows (lane (nn, g): Q[q0 + nn][32j + 8g ..], converted to fp16 once): lane (nn, g) ends up
//                   with the scores of query q0 + nn at positions pos0 + 16t + 4g + r (t = 0, 1; r = 0..3)
//   softmax         per query = per nn: 8 values per lane, reduced over g with two xor-shuffles; running (m, l)
//   O += P . V      the 8 probabilities a lane holds ARE its A operand if MFMA k-slot 8g + i is read as position
//                   16 (i >> 2) + 4g + (i & 3) — the product does not care how k is enumerated as long as B agrees, so
//                   no data moves between lanes.  B = V in that enumeration: V^T[d][pos] staged once per block and
//                   workgroup in LDS (coalesced 16-byte global reads, transposed 2-byte LDS writes), read back as two
//                   8-byte runs (positions 4g..4g+3 and 16+4g..) per 16-column output tile
// The accumulator rows of a lane (queries q0 + 4g + r) differ from the query its softmax state belongs to (q0 + nn):
// the rescale factors travel by __shfl from lane 4g + r.  fp16 operands, fp32 scores / statistics / accumulators.
// ============================================================================================================
typedef _Float16 ahalf8_t __attribute__((ext_vector_type(8)));
typedef _Float16 ahalf4_t __attribute__((ext_vector_type(4)));
typedef float afloatx4 __attribute__((ext_vector_type(4)));
constexpr int kAttnKB = 64;           // kv positions per block (32: two barriers and one softmax update per 32 keys)
constexpr int kAttnVStr = kAttnKB + 4;  // halves per V^T row in LDS: keeps the 8-byte reads aligned, skews banks

template <int HS>
__global__ __launch_bounds__(256) void attn_mfma_kernel(const AttnParams p) {
  constexpr int NJ = HS / 32, NDT = HS / 16, CH = HS / 8;  // k-slices of QK^T, output column tiles, V halves per thread
  __shared__ __attribute__((aligned(16))) _Float16 vt[HS * kAttnVStr];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, nn = l & 15, g = l >> 4;
  const int ihn = blockIdx.y, ibs = blockIdx.z;
  const int ihkv = ihn / (p.head_num / p.heads_kv);
  const bool causal = (p.flags & NS_ATTN_FLAG_IS_CAUSAL) != 0;
  // causal: the LAST query block sees the most keys — dispatch it first, so that the light blocks fill the tail of the
  // launch (in natural order the 32-block tiles of a 2048-token prompt started last and the kernel took twice its
  // average workgroup time, profiles/r02t_attn_prefill.txt)
  const int qblk = causal ? int(gridDim.x) - 1 - int(blockIdx.x) : int(blockIdx.x);
  const int off = p.sl_kv - p.sl_q;
  const int q0 = qblk * 64 + w * 16;
  const float* qb = p.q + ibs * p.step_q_bs + ihn * p.step_q_head_num;
  const _Float16* kb = p.k + ibs * p.step_k_bs + ihkv * p.step_k_head_num;
  const _Float16* vb = p.v + ibs * p.step_v_bs + ihkv * p.step_v_head_num;
  float* db = p.dst + ibs * p.step_dst_bs + ihn * p.step_dst_head_num;

  ahalf8_t qf[NJ];
  {
    const float* qr = qb + (long long)min(q0 + nn, p.sl_q - 1) * p.step_q_sl + 8 * g;
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int i = 0; i < 8; i++) qf[j][i] = (_Float16)qr[32 * j + i];
  }
  afloatx4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; dt++) o[dt] = afloatx4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const float sc = p.qk_scale * 1.4426950408889634f;  // scores in the exp2 domain
  const int q_last = min(qblk * 64 + 63, p.sl_q - 1);
  const int kv_end = causal ? min(p.sl_kv, q_last + off + 1) : p.sl_kv;            // workgroup-uniform
  const int visible = min(p.sl_kv, causal ? q0 + nn + off + 1 : p.sl_kv);          // mha_dense_wrapper.h:1440-1441
  const int vis_wave = min(p.sl_kv, causal ? q0 + off + 1 : p.sl_kv);              // what the wave's FIRST row sees

  constexpr int NT = kAttnKB / 16, NH = kAttnKB / 32;  // score tiles, 32-deep P.V slices per block
  // The K fragments and the V rows of block b + 1 are requested BEFORE block b is multiplied: without that every block
  // paid two exposed global round trips (K in front of the score MFMAs, V behind the first barrier) — 10 us per 64-key
  // block and workgroup, 110 TFLOPS at 2048 tokens, whatever the block size (profiles/r02t_attn_prefill.txt).
  typedef _Float16 ahalf2_t __attribute__((ext_vector_type(2)));
  const int vp = (tid >> 3) * 2, vc = tid & 7;  // V^T staging: this thread's two neighbouring positions, its CH head dims
  ahalf8_t kn[NT][NJ], vn[2][CH / 8];
  // (one register set each: the next K fragments are requested right behind the score MFMAs that consumed the current
  // ones, the next V rows right behind the LDS stores of the current ones)
  // row pointers advance by a uniform stride per block; only a block that reaches past the last key clamps its rows
  // (64-bit multiplies per row and block were a fifth of this loop's VALU work)
  const long long kstep_blk = (long long)kAttnKB * p.step_k_sl, vstep_blk = (long long)kAttnKB * p.step_v_sl;
  const _Float16* kp[NT];
  const _Float16* vpp[2];
#pragma unroll
  for (int t = 0; t < NT; t++) kp[t] = kb + (long long)(16 * t + nn) * p.step_k_sl + 8 * g;
#pragma unroll
  for (int q2 = 0; q2 < 2; q2++) vpp[q2] = vb + (long long)(vp + q2) * p.step_v_sl + vc * CH;
  auto fetch_k = [&](int pos0) {
    if (pos0 + kAttnKB <= p.sl_kv) {  // workgroup-uniform
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int j = 0; j < NJ; j++) kn[t][j] = *reinterpret_cast<const ahalf8_t*>(kp[t] + 32 * j);
    } else {
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const _Float16* kr = kb + (long long)min(pos0 + 16 * t + nn, p.sl_kv - 1) * p.step_k_sl + 8 * g;
#pragma unroll
        for (int j = 0; j < NJ; j++) kn[t][j] = *reinterpret_cast<const ahalf8_t*>(kr + 32 * j);
      }
    }
#pragma unroll
    for (int t = 0; t < NT; t++) kp[t] += kstep_blk;
  };
  auto fetch_v = [&](int pos0) {
    if (pos0 + kAttnKB <= p.sl_kv) {
#pragma unroll
      for (int q2 = 0; q2 < 2; q2++)
#pragma unroll
        for (int u = 0; u < CH / 8; u++) vn[q2][u] = *reinterpret_cast<const ahalf8_t*>(vpp[q2] + 8 * u);
    } else {
#pragma unroll
      for (int q2 = 0; q2 < 2; q2++) {
        const _Float16* vr = vb + (long long)min(pos0 + vp + q2, p.sl_kv - 1) * p.step_v_sl + vc * CH;
#pragma unroll
        for (int u = 0; u < CH / 8; u++) vn[q2][u] = *reinterpret_cast<const ahalf8_t*>(vr + 8 * u);
      }
    }
#pragma unroll
    for (int q2 = 0; q2 < 2; q2++) vpp[q2] += vstep_blk;
  };
  if (kv_end > 0) {
    fetch_k(0);
    fetch_v(0);
  }
  for (int pos0 = 0; pos0 < kv_end; pos0 += kAttnKB) {
    const bool more = pos0 + kAttnKB < kv_end;
    afloatx4 sv[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {
      sv[t] = afloatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NJ; j++) sv[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kn[t][j], qf[j], sv[t], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (more) fetch_k(pos0 + kAttnKB);
    __builtin_amdgcn_sched_barrier(0);
    float x[4 * NT], mx = -INFINITY;
    if (pos0 + kAttnKB <= vis_wave) {  // wave-uniform: every row of this wave sees the whole block (all but the diagonal)
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
    ahalf8_t pf[NH];  // slice h covers positions pos0 + 32 h ..: k-slot 8g + i <-> position 32 h + 16 (i >> 2) + 4g + (i & 3)
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
      if (pos0 + kAttnKB <= p.sl_kv) {
#pragma unroll
        for (int i = 0; i < CH; i++)
          *reinterpret_cast<ahalf2_t*>(vt + (vc * CH + i) * kAttnVStr + vp) = ahalf2_t{vn[0][i >> 3][i & 7], vn[1][i >> 3][i & 7]};
      } else {
        const bool ok0 = pos0 + vp < p.sl_kv, ok1 = pos0 + vp + 1 < p.sl_kv;
#pragma unroll
        for (int i = 0; i < CH; i++) {
          const _Float16 a0 = ok0 ? vn[0][i >> 3][i & 7] : (_Float16)0.f, a1 = ok1 ? vn[1][i >> 3][i & 7] : (_Float16)0.f;
          *reinterpret_cast<ahalf2_t*>(vt + (vc * CH + i) * kAttnVStr + vp) = ahalf2_t{a0, a1};
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (more) fetch_v(pos0 + kAttnKB);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) {
#pragma unroll
      for (int r = 0; r < 4; r++) o[dt][r] *= ar[r];
#pragma unroll
      for (int h = 0; h < NH; h++) {
        const _Float16* vr = vt + (16 * dt + nn) * kAttnVStr + 32 * h + 4 * g;
        const ahalf4_t lo = *reinterpret_cast<const ahalf4_t*>(vr), hi = *reinterpret_cast<const ahalf4_t*>(vr + 16);
        const ahalf8_t vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf[h], vf, o[dt], 0, 0, 0);
      }
    }
  }
  const float inv = l_run > 0.f ? p.out_scale / l_run : 0.f;
  float ir[4];
#pragma unroll
  for (int r = 0; r < 4; r++) ir[r] = __shfl(inv, 4 * g + r, 64);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = q0 + 4 * g + r;
    if (row >= p.sl_q) continue;
    float* dr = db + (long long)row * p.step_dst_sl + nn;
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) {
      float y = o[dt][r] * ir[r];
      // (y is the fp32 value from here on: without this hipcc folds product and conversion into one v_fma_mixlo_f16, and the shadow is the rounding of
      // the exact product instead of the rounding of what dst holds — a last fp16 bit apart now and then)
      if (p.dst16) asm volatile("" : "+v"(y));
      dr[16 * dt] = y;
      if (p.dst16) p.dst16[dr - p.dst + 16 * dt] = (_Float16)y;
    }
  }
}

// ============================================================================================================
// attn_mfma2_kernel (round 4) — prefill on the matrix cores, second generation: 128 query rows per workgroup, 32 per wave,
// v_mfma_f32_32x32x16_f16, K and V tiles of 64 keys staged ONCE per workgroup in LDS (two stages: the next tile travels
// global -> registers while the current one is multiplied, registers -> LDS behind the P.V products, one barrier per tile).
//   S^T = K . Q^T   A = K rows from LDS (lane (key l & 31, half h = l >> 5): 16 bytes K[key][16 j + 8 h ..]; the 16-byte slots of a
//                   row are XOR-swizzled by the row so that the 16 lanes of a ds_read_b128 group hit 16 distinct slots),
//                   B = Q rows in registers (fp16, converted once).  Lane (query n = l & 31, h) receives the scores of ITS query at
//                   keys (i & 3) + 8 (i >> 2) + 4 h of the 32-key tile, i = 0..15: softmax needs one exchange (lane ^ 32) per tile
//                   for the maximum; row sums stay per lane until the end.
//   O^T += V^T . P^T  A = V^T, B = P^T: the 8 probabilities i = 8 s .. 8 s + 7 a lane holds ARE its B operand of 16-deep step s if
//                   k-slot 8 h + i' is read as key 16 s + (i' & 3) + 8 (i' >> 2) + 4 h — no data moves between lanes — and the
//                   accumulators of a lane all belong to its own query: the rescale is lane-local.  A in that enumeration = two runs
//                   of 4 consecutive keys at one head dim: ds_read_b64_tr_b16 (the CDNA4 transposing LDS read) from a ROW-major
//                   image, [16-dim subtile][key][16 dims] with the subtiles 128 B off a 256 B multiple (the two 16-lane halves of
//                   a read then cover disjoint banks).
// Causal balance: all workgroups of a prompt are resident at once (2 per CU at 2048 x 32 heads), so the launch order cannot
// balance; the first half of the grid takes its query blocks heaviest-first, the second half lightest-first: the two
// workgroups that meet on a CU sum to the same work.  fp16 operands, fp32 scores / statistics / accumulators.
// ============================================================================================================
typedef float afloatx16 __attribute__((ext_vector_type(16)));
typedef short ashort4_t __attribute__((ext_vector_type(4)));
#ifndef NS_A2_ABL
#define NS_A2_ABL 0  // timing ablations (diagnostic builds, wrong results): 1 no softmax, 2 no P.V, 3 no K.Q^T, 4 no tile traffic, 5 = 4 + no barrier
#endif

// SB: the scores are biased before the softmax — ALiBi (+ key position x the head's slope, mha_dense_wrapper.h:1418-1447) and / or the
// 30 tanh(s / 30) soft cap — as attn_split_kernel applies them; a separate instantiation, the plain kernel's loop is unchanged.
// RG: 32-row groups per wave.  1 is what ships.  2 (256 query rows per workgroup: every K / V operand read from LDS feeds two MFMAs, the
// tile traffic is spread over twice the rows; all 512 registers, one wave per SIMD) was built, is correct (the whole attention suite and the
// shape fuzz pass on it) and is SLOWER: 4096 tokens 0.484 vs 0.268 ms, 8192 1.44 vs 0.85, 16384 4.89 vs 2.95 (profiles/r04bg_*) — two
// co-resident waves per SIMD hide more than halving the LDS traffic saves, and the 128-wide form spills 24 registers.
// PAGED (ns_hip_attn_prefill_paged; argument block AttnPrefillPagedParams, ns_attn.h): prompt-sized query blocks over a paged cache.  A unit is a
// (head, REQUEST) with its own packed query rows (q_start[b] ..) and its own live keys (kv_lens[b] + kdelta): the query blocks the request does not
// have leave in front of any barrier, sl_q / sl_kv of everything below are the request's q_len / kv_len, and every staged K / V row comes from the
// pools through that row's own table entry (attn_prefill_tile_key, attn_page_at: -1 is a load that is not issued and a register of zeros).  The
// entries of tile b + 1 are requested in front of tile b's K / V loads and held in one register, so no K / V load waits for a table lookup except the
// first tile's.  The arithmetic is the uniform body's, operation for operation; the uniform instantiations hold the instructions they held without
// it (docs/kernels/attention.md, "Prompt-sized query blocks over a paged cache").
__device__ __forceinline__ const AttnParams& attn_params_of(const AttnParams& p) { return p; }
__device__ __forceinline__ const AttnParams& attn_params_of(const AttnPrefillPagedParams& pp) { return pp.a; }
template <int HS, bool SB, bool PAD, int RG = 1, bool PAGED = false>
__device__ __forceinline__ void attn_mfma2_body(const std::conditional_t<PAGED, AttnPrefillPagedParams, AttnParams>& pp, const int nqb, const int aligned_dst,
                                                const int xcd_map) {
  const AttnParams& p = attn_params_of(pp);
  constexpr int NJ = HS / 16, NDT = HS / 32, NCH = HS / 8, KROW = HS * 2, NSUB = HS / 16;
  constexpr int KTILE = kA2KB * KROW, STAGE = a2_stage_bytes<HS>();
  constexpr int KU = NCH / 4;               // 16-byte K chunks per thread and tile
  // a wave-wide V load: lane = (half of a 32-byte subtile row, row of a group of VRG, subtile, group); 8 consecutive lanes write
  // 128 contiguous LDS bytes of one subtile (head size 256: two runs of 64 in neighbouring subtiles)
  constexpr int VRG = NSUB <= 8 ? 4 : 2, VRGL = NSUB <= 8 ? 2 : 1;
  constexpr int VRW = VRG * (32 / VRG / NSUB);  // V rows per wave-wide load
  constexpr int VU = kA2KB / (4 * VRW);         // V chunks per thread and tile
  extern __shared__ __attribute__((aligned(16))) unsigned char smem2[];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 31, h = l >> 5;
  const bool causal = (p.flags & NS_ATTN_FLAG_IS_CAUSAL) != 0;
  // workgroup -> (query block, head, batch).  Workgroups go to the XCDs round-robin (id % 8) and each XCD has its own L2: with the
  // plain order every XCD walks every head's K / V (32 MB at 2048 x 32 heads against 4 MB of L2 — the kernel then streams K / V from
  // memory at ~4 TB/s and is bound by that).  xcd_map: all query blocks of a kv head (and of the query heads sharing it) on ONE XCD,
  // head after head, so a head's K / V is fetched from memory once and re-read from that L2.
  // Causal balance: every (head, batch) unit walks its query blocks in ONE direction; the first half of the units (of the XCD's list)
  // heaviest-first, the second half lightest-first.
  const unsigned G = unsigned(p.head_num / p.heads_kv), units = gridDim.x / unsigned(nqb);
  unsigned unit = blockIdx.x / unsigned(nqb), ordn = blockIdx.x % unsigned(nqb);
  bool heavy_first = unit < (units + 1) / 2;
  if (xcd_map) {
    const unsigned x = blockIdx.x & 7u, sl = blockIdx.x >> 3;  // XCD, index inside the XCD's list
    const unsigned ul = sl / unsigned(nqb);                     // the XCD's ul-th (kv head, query head of its group)
    ordn = sl % unsigned(nqb);
    unit = ((ul / G) * 8u + x) * G + ul % G;
    heavy_first = ul < (units / 8u + 1) / 2;
  }
  const int hb = int(unit);
  const int qblk = causal && heavy_first ? nqb - 1 - int(ordn) : int(ordn);
  const int ihn = hb % p.head_num, ibs = hb / p.head_num;
  const int ihkv = ihn / (p.head_num / p.heads_kv);
  constexpr int WGR = 128 * RG;  // query rows per workgroup
  // PAGED: the request's own geometry — its packed query rows, its live keys
  int q_base = 0, q_len = 0, kv_len = 0;
  if constexpr (PAGED) {
    q_base = pp.q_start[ibs];
    q_len = attn_block_q_len(pp.q_start, ibs, p.sl_q);
    kv_len = attn_prefill_kv_len(pp.kv_lens, ibs, pp.kdelta, p.sl_kv);
    if (qblk * WGR >= q_len) return;  // no row of this query block is a row of the request (workgroup-uniform, in front of any barrier)
  }
  // (read where they are used, so that the uniform instantiations hold the instructions they held without the PAGED ones)
  auto sl_q = [&] { if constexpr (PAGED) return q_len; else return p.sl_q; };
  auto sl_kv = [&] { if constexpr (PAGED) return kv_len; else return p.sl_kv; };
  const int off = sl_kv() - sl_q();
  const int q0 = qblk * WGR + w * (32 * RG);
  const float* qb = p.q + ibs * p.step_q_bs + ihn * p.step_q_head_num;  // (PAGED: packed rows and the pools — the plan's batch steps are 0)
  const _Float16* kb = p.k + ibs * p.step_k_bs + ihkv * p.step_k_head_num;
  const _Float16* vb = p.v + ibs * p.step_v_bs + ihkv * p.step_v_head_num;
  float* db = p.dst + ibs * p.step_dst_bs + ihn * p.step_dst_head_num;
  if constexpr (PAGED) qb += (long long)q_base * p.step_q_sl, db += (long long)q_base * p.step_dst_sl;

  // PAD: HS is the PADDED head size of this instantiation (64 / 128 / 256) and the call's own head size hs < HS a multiple of 8:
  // query dims, K / V chunks and output dims from hs on are zeros / never stored (head sizes 80, 96, 112, 160, 192 ... ride on the
  // next size up; a separate instantiation: the predicates cost the exact sizes a third of their speed)
  const int hs = PAD ? p.head_size : HS;
  ahalf8_t qf[RG][NJ];
  afloatx16 o[RG][NDT];
  float m_run[RG], l_run[RG];  // l_run: this lane's half of the row sum
#pragma unroll
  for (int rg = 0; rg < RG; rg++) {
    const float* qr = qb + (long long)min(q0 + 32 * rg + n, sl_q() - 1) * p.step_q_sl + 8 * h;
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int i = 0; i < 8; i++) qf[rg][j][i] = 16 * j + 8 * h < hs ? (_Float16)qr[16 * j + i] : (_Float16)0.f;
#pragma unroll
    for (int dt = 0; dt < NDT; dt++)
#pragma unroll
      for (int i = 0; i < 16; i++) o[rg][dt][i] = 0.f;
    m_run[rg] = -INFINITY, l_run[rg] = 0.f;
  }
  const float sc = SB ? 1.f : p.qk_scale * 1.4426950408889634f;  // scores in the exp2 domain (SB: the biased scores are scaled up front)
  float slope = 0.f;
  const bool tanh30 = SB && (p.flags & NS_ATTN_FLAG_IS_TANH30) != 0;
  if (SB && (p.flags & NS_ATTN_FLAG_IS_ALIBI8) != 0) {
    const int gh = ihn + p.alibi_head_off;
    slope = gh < p.alibi_log2_floor ? powf(p.alibi_m0, float(gh + 1)) : powf(p.alibi_m1, float(2 * (gh - p.alibi_log2_floor) + 1));
  }
  const int q_last_wg = min(qblk * WGR + WGR - 1, sl_q() - 1);
  const int kv_end = causal ? min(sl_kv(), q_last_wg + off + 1) : sl_kv();                     // workgroup-uniform
  int visible[RG];                                                                             // mha_dense_wrapper.h:1440-1441
#pragma unroll
  for (int rg = 0; rg < RG; rg++) visible[rg] = min(sl_kv(), causal ? min(q0 + 32 * rg + n, sl_q() - 1) + off + 1 : sl_kv());
  const int vis_first = min(sl_kv(), causal ? q0 + off + 1 : sl_kv());                          // the wave's first row
  const int vis_last = min(sl_kv(), causal ? min(q0 + 32 * RG - 1, sl_q() - 1) + off + 1 : sl_kv());  // the wave's last row
  const bool wave_live = q0 < sl_q();

  // ---- tile staging: global -> registers -> LDS ----
  ahalf8_t kst[KU], vst[VU];
  int krow[KU], kslot[KU], vrow[VU];
#pragma unroll
  for (int u = 0; u < KU; u++) {
    const int id = tid + 256 * u;
    krow[u] = id / NCH;
    const int c = id % NCH;
    const int swz = HS >= 128 ? (krow[u] & 15) : ((krow[u] >> 1) & 7);
    kslot[u] = krow[u] * KROW + ((c ^ swz) << 4);
  }
  const int vsub = (l >> (1 + VRGL)) % NSUB, vrq = (l >> (1 + VRGL)) / NSUB, vr = (l >> 1) & (VRG - 1), vhf = l & 1;
#pragma unroll
  for (int u = 0; u < VU; u++) vrow[u] = u * (4 * VRW) + w * VRW + vrq * VRG + vr;
  const int kcol = (tid % NCH) * 8, vcol = 16 * vsub + 8 * vhf;
  // row pointers advance by a uniform stride per tile; only the tile that reaches past the last key clamps its rows
  const _Float16* kp0 = kb + (long long)krow[0] * p.step_k_sl + kcol;
  const _Float16* vp0 = vb + (long long)vrow[0] * p.step_v_sl + vcol;
  const long long ku_step = (long long)(256 / NCH) * p.step_k_sl, vu_step = (long long)(4 * VRW) * p.step_v_sl;
  const long long ktile_step = (long long)kA2KB * p.step_k_sl, vtile_step = (long long)kA2KB * p.step_v_sl;
  const bool k_in = !PAD || kcol < hs, v_in = !PAD || vcol < hs;  // this thread's 16-byte column of the rows exists (else: zeros, once)
  if (!k_in) {
#pragma unroll
    for (int u = 0; u < KU; u++) kst[u] = ahalf8_t{0, 0, 0, 0, 0, 0, 0, 0};
  }
  if (!v_in) {
#pragma unroll
    for (int u = 0; u < VU; u++) vst[u] = ahalf8_t{0, 0, 0, 0, 0, 0, 0, 0};
  }
  // PAGED: one table entry per wave and staging step u, for K and V alike — the rows a wave stages at step u, K's and V's, are the aligned group of
  // 16 / KU rows from tile row u * (64 / KU) + w * (16 / KU) on; a page holds 16 keys or more and tiles start at multiples of 64, so the keys the
  // group's rows clamp to (attn_prefill_tile_key) all lie in the page of the key its FIRST row clamps to.  Lane l of a wave fetches the entry of step
  // l % KU into ONE register (a vector load: it retires with the K / V loads issued behind it, which park() waits for anyway — a scalar load would
  // share its counter with the LDS reads of the tile's products and stall them); step u reads it from lane u.  idv holds the entries of the tile
  // the NEXT fetch requests (kv_len >= 1 wherever a tile is fetched: nb > 0).
  static_assert(!PAGED || (KU == VU && 256 / NCH == 4 * VRW), "K and V rows of a staging step: the same group of a wave");
  int idv = 0;
  const int grp_l = (l % KU) * (64 / KU) + w * (16 / KU);  // first tile row of the group whose entry this lane fetches
  auto fetch_ids = [&](int pos0) {
    if constexpr (PAGED) return pp.pg.table[(long long)ibs * pp.pg.table_stride + (attn_prefill_tile_key(pos0, grp_l, kv_len) >> pp.pg.block_shift)];
    return 0;
  };
  auto fetch_paged = [&](int pos0) {
    if constexpr (PAGED) {
      const int idv_n = fetch_ids(pos0 + kA2KB);  // (clamped to the last live key: a valid entry also behind the last tile)
#pragma unroll
      for (int u = 0; u < KU; u++) {
        const int id = __builtin_amdgcn_readlane(idv, u);
        if (k_in) {
          const long long cell = attn_page_at(pp.pg, id, attn_prefill_tile_key(pos0, krow[u], kv_len), p.step_k_sl);
          kst[u] = cell >= 0 ? *reinterpret_cast<const ahalf8_t*>(kb + cell + kcol) : ahalf8_t{0, 0, 0, 0, 0, 0, 0, 0};
        }
        if (v_in) {
          const long long cell = attn_page_at(pp.pg, id, attn_prefill_tile_key(pos0, vrow[u], kv_len), p.step_v_sl);
          vst[u] = cell >= 0 ? *reinterpret_cast<const ahalf8_t*>(vb + cell + vcol) : ahalf8_t{0, 0, 0, 0, 0, 0, 0, 0};
        }
      }
      idv = idv_n;
    }
  };
  auto fetch = [&](int pos0) {
    if constexpr (PAGED) return fetch_paged(pos0);
    if (pos0 + kA2KB <= p.sl_kv) {  // workgroup-uniform
      if (k_in) {
#pragma unroll
        for (int u = 0; u < KU; u++) kst[u] = *reinterpret_cast<const ahalf8_t*>(kp0 + u * ku_step);
      }
      if (v_in) {
#pragma unroll
        for (int u = 0; u < VU; u++) vst[u] = *reinterpret_cast<const ahalf8_t*>(vp0 + u * vu_step);
      }
    } else {
      if (k_in) {
#pragma unroll
        for (int u = 0; u < KU; u++)
          kst[u] = *reinterpret_cast<const ahalf8_t*>(kb + (long long)min(pos0 + krow[u], p.sl_kv - 1) * p.step_k_sl + kcol);
      }
      if (v_in) {
#pragma unroll
        for (int u = 0; u < VU; u++)
          vst[u] = *reinterpret_cast<const ahalf8_t*>(vb + (long long)min(pos0 + vrow[u], p.sl_kv - 1) * p.step_v_sl + vcol);
      }
    }
    kp0 += ktile_step;
    vp0 += vtile_step;
  };
  auto park = [&](int stage) {
    unsigned char* sb = smem2 + stage * STAGE;
#pragma unroll
    for (int u = 0; u < KU; u++) *reinterpret_cast<ahalf8_t*>(sb + kslot[u]) = kst[u];
#pragma unroll
    for (int u = 0; u < VU; u++) *reinterpret_cast<ahalf8_t*>(sb + KTILE + vsub * kA2VSub + vrow[u] * 32 + vhf * 16) = vst[u];
  };
  // operand addresses inside a stage
  const int swz_n = HS >= 128 ? (n & 15) : ((n >> 1) & 7);
  const int k_rd = n * KROW;                                                        // + 32 T rows, slot (2 j + h) ^ swizzle
  const int v_rd = KTILE + ((l >> 4) & 1) * kA2VSub + (4 * h + ((l & 15) >> 2)) * 32 + (l & 3) * 8;  // + 2 dt subtiles, + (32 T + 16 s) rows, + 8 rows

  const int nb = (kv_end + kA2KB - 1) / kA2KB;
  if (nb > 0) {
    idv = fetch_ids(0);
    fetch(0);
    park(0);
  }
  __syncthreads();
  for (int b = 0; b < nb; b++) {
    const int pos0 = b * kA2KB;
    const unsigned char* sb = smem2 + (b & 1) * STAGE;
    if (b + 1 < nb && NS_A2_ABL < 4) fetch(pos0 + kA2KB);
    if (wave_live && pos0 < vis_last) {
      // operands travel LDS -> registers one group of four MFMAs ahead of their use (two register sets, fenced: left alone hipcc
      // re-uses ONE operand register and serialises read -> wait -> MFMA, ~100 exposed cycles per MFMA)
      afloatx16 sv[RG][2];
#pragma unroll
      for (int rg = 0; rg < RG; rg++)
#pragma unroll
        for (int T = 0; T < 2; T++)
#pragma unroll
          for (int i = 0; i < 16; i++) sv[rg][T][i] = 0.f;
      {
        constexpr int CPT = NJ / 4, NCK = 2 * CPT;  // groups per 32-key tile, groups per block
        ahalf8_t kf[2][4];
        auto ldk = [&](int c, ahalf8_t(&dst)[4]) {
          const int T = c / CPT, j0 = (c % CPT) * 4;
#pragma unroll
          for (int u = 0; u < 4; u++)
            dst[u] = *reinterpret_cast<const ahalf8_t*>(sb + k_rd + 32 * T * KROW + (((2 * (j0 + u) + h) ^ swz_n) << 4));
        };
        if (NS_A2_ABL != 3) ldk(0, kf[0]);
#pragma unroll
        for (int c = 0; c < (NS_A2_ABL == 3 ? 0 : NCK); c++) {
          if (c + 1 < NCK) ldk(c + 1, kf[(c + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < 4; u++)
#pragma unroll
            for (int rg = 0; rg < RG; rg++)
              sv[rg][c / CPT] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[c & 1][u], qf[rg][(c % CPT) * 4 + u], sv[rg][c / CPT], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // softmax in the exp2 domain on the raw scores (sc > 0: the launcher sends other scales to the 64-row kernel): p = exp2(s sc - m sc)
      // is one fused multiply-add and one v_exp_f32 per score; the running maximum is kept unscaled
      ahalf8_t pf[RG][4];  // (T, s) -> 2 T + s
#pragma unroll
      for (int rg = 0; rg < RG; rg++) {
#if NS_A2_ABL == 1
#pragma unroll
      for (int e = 0; e < 32; e++) pf[rg][e >> 3][e & 7] = (_Float16)sv[rg][e >> 4][e & 15];
      l_run[rg] += 1.f;
#else
      if constexpr (SB) {
#pragma unroll
        for (int e = 0; e < 32; e++) {
          const int i = e & 15;
          const int pos = pos0 + 32 * (e >> 4) + (i & 3) + 8 * (i >> 2) + 4 * h;
          float v = sv[rg][e >> 4][i] * p.qk_scale;
          if (tanh30) v = 30.f * tanhf(v * (1.f / 30.f));
          v += float(pos) * slope;
          sv[rg][e >> 4][i] = v * 1.4426950408889634f;
        }
      }
      if (pos0 + kA2KB > vis_first) {  // wave-uniform: only tiles on the diagonal / past the last key are masked
#pragma unroll
        for (int e = 0; e < 32; e++) {
          const int i = e & 15;
          const int pos = pos0 + 32 * (e >> 4) + (i & 3) + 8 * (i >> 2) + 4 * h;
          if (pos >= visible[rg]) sv[rg][e >> 4][i] = -INFINITY;
        }
      }
      float mx = sv[rg][0][0];
#pragma unroll
      for (int e = 1; e < 32; e++) mx = fmaxf(mx, sv[rg][e >> 4][e & 15]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run[rg], mx);
      const float neg_m = m_new == -INFINITY ? 0.f : -m_new * sc;  // nothing visible yet: every exp2 below is exp2(-inf) = 0
      const float alpha = __builtin_amdgcn_exp2f(fmaf(m_run[rg], sc, neg_m));
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < 32; e++) {
        const float pe = __builtin_amdgcn_exp2f(fmaf(sv[rg][e >> 4][e & 15], sc, neg_m));
        ps += pe;
        pf[rg][e >> 3][e & 7] = (_Float16)pe;
      }
      l_run[rg] = l_run[rg] * alpha + ps;
      m_run[rg] = m_new;
      if (__any(alpha != 1.f)) {
#pragma unroll
        for (int dt = 0; dt < NDT; dt++)
#pragma unroll
          for (int i = 0; i < 16; i++) o[rg][dt][i] *= alpha;
      }
#endif
      }
      {
        ahalf8_t vf[2][4];
        auto ldv = [&](int dt, ahalf8_t(&dst)[4]) {
#pragma unroll
          for (int ts = 0; ts < 4; ts++) {
            const unsigned char* va = sb + v_rd + 2 * dt * kA2VSub + 16 * ts * 32;
            const ashort4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ashort4_t __attribute__((address_space(3)))*)(va));
            const ashort4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ashort4_t __attribute__((address_space(3)))*)(va + 8 * 32));
            dst[ts] = __builtin_bit_cast(ahalf8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
          }
        };
        if (NS_A2_ABL != 2) ldv(0, vf[0]);
#pragma unroll
        for (int dt = 0; dt < (NS_A2_ABL == 2 ? 0 : NDT); dt++) {
          if (dt + 1 < NDT) ldv(dt + 1, vf[(dt + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int ts = 0; ts < 4; ts++)
#pragma unroll
            for (int rg = 0; rg < RG; rg++) o[rg][dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[dt & 1][ts], pf[rg][ts], o[rg][dt], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    if (b + 1 < nb && NS_A2_ABL < 4) park((b + 1) & 1);
    if (NS_A2_ABL < 5) __syncthreads();
  }
#pragma unroll
  for (int rg = 0; rg < RG; rg++) {
  l_run[rg] += __shfl_xor(l_run[rg], 32, 64);
  const float inv = l_run[rg] > 0.f ? p.out_scale / l_run[rg] : 0.f;
  const int row = q0 + 32 * rg + n;
  if (row < sl_q()) {
    float* dr = db + (long long)row * p.step_dst_sl;
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) {
#pragma unroll
      for (int bq = 0; bq < 4; bq++) {
        const int d = 32 * dt + 8 * bq + 4 * h;
        if (PAD && d >= hs) continue;
        const afloatx4 y = afloatx4{o[rg][dt][4 * bq] * inv, o[rg][dt][4 * bq + 1] * inv, o[rg][dt][4 * bq + 2] * inv, o[rg][dt][4 * bq + 3] * inv};
        if (aligned_dst) {
          *reinterpret_cast<afloatx4*>(dr + d) = y;
          if (p.dst16) *reinterpret_cast<ahalf4_t*>(p.dst16 + (dr - p.dst) + d) = ahalf4_t{(_Float16)y[0], (_Float16)y[1], (_Float16)y[2], (_Float16)y[3]};
        } else {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            dr[d + r] = y[r];
            if (p.dst16) p.dst16[(dr - p.dst) + d + r] = (_Float16)y[r];
          }
        }
      }
    }
  }
  }
}

// ============================================================================================================
// attn_mfma3_kernel (round 6) — the operands, layouts and arithmetic of attn_mfma2_kernel (exact head sizes 64 / 128, no score bias) with the K / V tiles
// travelling HBM -> LDS by DMA (buffer_load ... lds, 1 KiB per wave-wide request): the XOR swizzle of a K row's 16-byte slots and the V subtile image are
// made by WHICH global 16 bytes a lane asks for (the DMA writes lane-linear), so there are no staging registers and no register -> LDS pass ("park") —
// 8 requests per wave and tile instead of 8 loads + 8 ds_write_b128 + their address arithmetic, and 32 registers free.  Rows past the last key lie outside
// the buffer descriptor and arrive as zeros (their scores are masked).  2048 tokens 500 -> 530 TFLOPS causal, 4096 545 -> 605, 8192 667 -> 750 (standalone,
// profiles/r06_attn_prefill_dma.txt); a layer's launch inside the 2048-token prompt -3 us.
// Built on top of it, correct (the whole attention suite passes) and NOT adopted: P.V lagging one tile so that its MFMAs issue between the exponentials of the
// next tile (sched_group_barrier pattern: one MFMA, two transposing LDS reads, two v_exp, ten VALU): the second set of probabilities pushes the 128-wide
// instantiation to 256 registers + 21 spilled, each MFMA waits for the LDS reads placed right in front of it — 410-439 TFLOPS at 2048 tokens against 530.
// Requesting the first V operands in front of the exponentials: also slower (504 vs 540).  What bounds 2048 tokens now is the pairing: a CU's two workgroups
// (heavy + light q-block: equal SUM of tiles) run together for the light one's tiles only, the heavy one then has its SIMDs to itself — 1.9 us per
// tile-unit against 1.41 at 8192 tokens, where eight workgroups per CU even that out.
template <int HS>
__device__ __forceinline__ void attn_mfma3_body(const AttnParams& p, const int nqb, const int aligned_dst, const int xcd_map) {
  constexpr int NJ = HS / 16, NDT = HS / 32, NCH = HS / 8, KROW = HS * 2, NSUB = HS / 16;
  constexpr int KTILE = kA2KB * KROW, VTILE = NSUB * kA2VSub;
  constexpr int KREQ = KTILE / 1024 / 4, VREQ = 2 * NSUB / 4;  // DMA requests per wave and tile
  extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];  // K[2][KTILE] | V[2][VTILE]
  using LdsPtr [[maybe_unused]] = __attribute__((address_space(3))) unsigned char*;  // (used by the device side only)
  const int tid = threadIdx.x, l = tid & 63, n = l & 31, h = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool causal = (p.flags & NS_ATTN_FLAG_IS_CAUSAL) != 0;
  const unsigned G = unsigned(p.head_num / p.heads_kv), units = gridDim.x / unsigned(nqb);
  unsigned unit = blockIdx.x / unsigned(nqb), ordn = blockIdx.x % unsigned(nqb);
  bool heavy_first = unit < (units + 1) / 2;
  if (xcd_map & 1) {
    const unsigned x = blockIdx.x & 7u, sl = blockIdx.x >> 3;
    const unsigned ul = sl / unsigned(nqb);
    ordn = sl % unsigned(nqb);
    unit = ((ul / G) * 8u + x) * G + ul % G;
    heavy_first = ul < (units / 8u + 1) / 2;
  }
  const int hb = int(unit);
  const int qblk = causal && heavy_first ? nqb - 1 - int(ordn) : int(ordn);
  const int ihn = hb % p.head_num, ibs = hb / p.head_num;
  const int ihkv = ihn / (p.head_num / p.heads_kv);
  const int off = p.sl_kv - p.sl_q;
  const int q0 = qblk * 128 + w * 32;
  const float* qb = p.q + ibs * p.step_q_bs + ihn * p.step_q_head_num;
  const _Float16* kb = p.k + ibs * p.step_k_bs + ihkv * p.step_k_head_num;
  const _Float16* vb = p.v + ibs * p.step_v_bs + ihkv * p.step_v_head_num;
  float* db = p.dst + ibs * p.step_dst_bs + ihn * p.step_dst_head_num;

  ahalf8_t qf[NJ];
  afloatx16 o[NDT];
  float m_run = -INFINITY, l_run = 0.f;
  {
    const float* qr = qb + (long long)min(q0 + n, p.sl_q - 1) * p.step_q_sl + 8 * h;
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int i = 0; i < 8; i++) qf[j][i] = (_Float16)qr[16 * j + i];
#pragma unroll
    for (int dt = 0; dt < NDT; dt++)
#pragma unroll
      for (int i = 0; i < 16; i++) o[dt][i] = 0.f;
  }
  const float sc = p.qk_scale * 1.4426950408889634f;
  const int q_last_wg = min(qblk * 128 + 127, p.sl_q - 1);
  const int kv_end = causal ? min(p.sl_kv, q_last_wg + off + 1) : p.sl_kv;
  const int visible = min(p.sl_kv, causal ? min(q0 + n, p.sl_q - 1) + off + 1 : p.sl_kv);
  const int vis_first = min(p.sl_kv, causal ? q0 + off + 1 : p.sl_kv);
  const int vis_last = min(p.sl_kv, causal ? min(q0 + 31, p.sl_q - 1) + off + 1 : p.sl_kv);
  const bool wave_live = q0 < p.sl_q;

  // ---- tile requests (DMA): descriptors over the head's rows; a row past the last key lies outside them and arrives as zeros (its scores are masked) ----
  auto uniform_ptr = [](const _Float16* ptr) {
    const uint64_t v = reinterpret_cast<uint64_t>(ptr);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(v)), hi = __builtin_amdgcn_readfirstlane(uint32_t(v >> 32));
    return reinterpret_cast<_Float16*>((uint64_t(hi) << 32) | lo);
  };
  const uint32_t k_bytes = uint32_t((size_t(p.sl_kv - 1) * p.step_k_sl + HS) * 2), v_bytes = uint32_t((size_t(p.sl_kv - 1) * p.step_v_sl + HS) * 2);
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(kb), 0, __builtin_amdgcn_readfirstlane(k_bytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(vb), 0, __builtin_amdgcn_readfirstlane(v_bytes), 0x00020000);
  uint32_t kvoff[KREQ], vvoff[VREQ];  // byte offsets inside tile 0 of what this lane asks for in its wave's u-th request
  constexpr int RPC = 1024 / KROW;    // K rows per 1 KiB request
#pragma unroll
  for (int u = 0; u < KREQ; u++) {
    const int r = (w * KREQ + u) * RPC + l / NCH, slot = l % NCH;
    const int swz = HS >= 128 ? (r & 15) : ((r >> 1) & 7);
    kvoff[u] = (uint32_t(r) * uint32_t(p.step_k_sl) + uint32_t((slot ^ swz) * 8)) * 2u;
  }
#pragma unroll
  for (int u = 0; u < VREQ; u++) {
    const int c = w * VREQ + u, sub = c >> 1, half = c & 1;  // request c = (subtile, rows 0..31 / 32..63)
    vvoff[u] = (uint32_t(half * 32 + (l >> 1)) * uint32_t(p.step_v_sl) + uint32_t(16 * sub + 8 * (l & 1))) * 2u;
  }
  const uint32_t ktile_step = uint32_t(kA2KB) * uint32_t(p.step_k_sl) * 2u, vtile_step = uint32_t(kA2KB) * uint32_t(p.step_v_sl) * 2u;
  auto issue_k = [&](int t, int buf) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int u = 0; u < KREQ; u++)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, reinterpret_cast<__attribute__((address_space(3))) void*>((LdsPtr)(smem3) + buf * KTILE + (w * KREQ + u) * 1024), 16,
                                               kvoff[u] + uint32_t(t) * ktile_step, 0, 0, 0);
#endif
  };
  auto issue_v = [&](int t, int buf) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int u = 0; u < VREQ; u++) {
      const int c = w * VREQ + u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, reinterpret_cast<__attribute__((address_space(3))) void*>((LdsPtr)(smem3) + 2 * KTILE + buf * VTILE + (c >> 1) * kA2VSub + (c & 1) * 1024),
                                               16, vvoff[u] + uint32_t(t) * vtile_step, 0, 0, 0);
    }
#endif
  };
  const int swz_n = HS >= 128 ? (n & 15) : ((n >> 1) & 7);
  const int k_rd = n * KROW;
  const int v_rd = ((l >> 4) & 1) * kA2VSub + (4 * h + ((l & 15) >> 2)) * 32 + (l & 3) * 8;

  // K(b) . Q^T -> sv (two 32-key halves), operands one group of four MFMAs ahead of their use
  auto qk = [&](const unsigned char* kt, afloatx16 (&sv)[2]) {
    constexpr int CPT = NJ / 4, NCK = 2 * CPT;
#pragma unroll
    for (int T = 0; T < 2; T++)
#pragma unroll
      for (int i = 0; i < 16; i++) sv[T][i] = 0.f;
    ahalf8_t kf[2][4];
    auto ldk = [&](int c, ahalf8_t(&dst)[4]) {
      const int T = c / CPT, j0 = (c % CPT) * 4;
#pragma unroll
      for (int u = 0; u < 4; u++) dst[u] = *reinterpret_cast<const ahalf8_t*>(kt + k_rd + 32 * T * KROW + (((2 * (j0 + u) + h) ^ swz_n) << 4));
    };
    ldk(0, kf[0]);
#pragma unroll
    for (int c = 0; c < NCK; c++) {
      if (c + 1 < NCK) ldk(c + 1, kf[(c + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; u++) sv[c / CPT] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[c & 1][u], qf[(c % CPT) * 4 + u], sv[c / CPT], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // the exponentials of a tile: scores -> probabilities (fp16, the B operand of P.V), running maximum / sum; returns the factor the accumulators take
  auto softmax = [&](afloatx16 (&sv)[2], ahalf8_t (&pf)[4], int pos0, bool masked) -> float {
    if (masked) {
#pragma unroll
      for (int e = 0; e < 32; e++) {
        const int i = e & 15;
        const int pos = pos0 + 32 * (e >> 4) + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (pos >= visible) sv[e >> 4][i] = -INFINITY;
      }
    }
    float mx = sv[0][0];
#pragma unroll
    for (int e = 1; e < 32; e++) mx = fmaxf(mx, sv[e >> 4][e & 15]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float neg_m = m_new == -INFINITY ? 0.f : -m_new * sc;
    const float alpha = __builtin_amdgcn_exp2f(fmaf(m_run, sc, neg_m));
    float ps = 0.f;
#pragma unroll
    for (int e = 0; e < 32; e++) {
      const float pe = __builtin_amdgcn_exp2f(fmaf(sv[e >> 4][e & 15], sc, neg_m));
      ps += pe;
      pf[e >> 3][e & 7] = (_Float16)pe;
    }
    l_run = l_run * alpha + ps;
    m_run = m_new;
    return alpha;
  };
  // O^T += V(t)^T . P^T, operands one group of four MFMAs ahead of their use
  auto pv = [&](const unsigned char* vt, const ahalf8_t (&pf)[4]) {
    auto ldv = [&](int dt, ahalf8_t(&dst)[4]) {
#pragma unroll
      for (int ts = 0; ts < 4; ts++) {
        const unsigned char* va = vt + v_rd + 2 * dt * kA2VSub + 16 * ts * 32;
        const ashort4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ashort4_t __attribute__((address_space(3)))*)(va));
        const ashort4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ashort4_t __attribute__((address_space(3)))*)(va + 8 * 32));
        dst[ts] = __builtin_bit_cast(ahalf8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      }
    };
    ahalf8_t vf[2][4];
    ldv(0, vf[0]);
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) {
      if (dt + 1 < NDT) ldv(dt + 1, vf[(dt + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ts = 0; ts < 4; ts++) o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[dt & 1][ts], pf[ts], o[dt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto rescale = [&](float alpha) {
    if (__any(alpha != 1.f)) {
#pragma unroll
      for (int dt = 0; dt < NDT; dt++)
#pragma unroll
        for (int i = 0; i < 16; i++) o[dt][i] *= alpha;
    }
  };

  const int nb = (kv_end + kA2KB - 1) / kA2KB;
  const int variant = xcd_map >> 8;  // bit 0: the next tile is requested behind K.Q^T instead of in front of it; bit 1: raised priority while K.Q^T issues
  if (nb > 0) issue_k(0, 0), issue_v(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int b = 0; b < nb; b++) {
    const int pos0 = b * kA2KB;
    const bool more = b + 1 < nb;
    if (!(variant & 1) && more) issue_k(b + 1, (b + 1) & 1), issue_v(b + 1, (b + 1) & 1);
    if (wave_live && pos0 < vis_last) {
      afloatx16 sv[2];
      ahalf8_t pf[4];
      if (variant & 2) __builtin_amdgcn_s_setprio(2);
      qk(smem3 + (b & 1) * KTILE, sv);
      if (variant & 2) __builtin_amdgcn_s_setprio(0);
      if ((variant & 1) && more) issue_k(b + 1, (b + 1) & 1), issue_v(b + 1, (b + 1) & 1);
      const float alpha = softmax(sv, pf, pos0, pos0 + kA2KB > vis_first);  // (masked: wave-uniform — only tiles on the diagonal / past the last key)
      rescale(alpha);
      pv(smem3 + 2 * KTILE + (b & 1) * VTILE, pf);
    } else if ((variant & 1) && more) {
      issue_k(b + 1, (b + 1) & 1), issue_v(b + 1, (b + 1) & 1);
    }
    // this wave's requests have landed; every wave is done with tile b's buffers
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  l_run += __shfl_xor(l_run, 32, 64);
  const float inv = l_run > 0.f ? p.out_scale / l_run : 0.f;
  const int row = q0 + n;
  if (row < p.sl_q) {
    float* dr = db + (long long)row * p.step_dst_sl;
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) {
#pragma unroll
      for (int bq = 0; bq < 4; bq++) {
        const int d = 32 * dt + 8 * bq + 4 * h;
        const afloatx4 y = afloatx4{o[dt][4 * bq] * inv, o[dt][4 * bq + 1] * inv, o[dt][4 * bq + 2] * inv, o[dt][4 * bq + 3] * inv};
        if (aligned_dst) {
          *reinterpret_cast<afloatx4*>(dr + d) = y;
          if (p.dst16) *reinterpret_cast<ahalf4_t*>(p.dst16 + (dr - p.dst) + d) = ahalf4_t{(_Float16)y[0], (_Float16)y[1], (_Float16)y[2], (_Float16)y[3]};
        } else {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            dr[d + r] = y[r];
            if (p.dst16) p.dst16[(dr - p.dst) + d + r] = (_Float16)y[r];
          }
        }
      }
    }
  }
}
template <int HS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_mfma3_kernel(const AttnParams p, const int nqb, const int aligned_dst, const int xcd_map) {
  attn_mfma3_body<HS>(p, nqb, aligned_dst, xcd_map);
}

template <int HS, bool SB = false, bool PAD = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_mfma2_kernel(const AttnParams p, const int nqb, const int aligned_dst, const int xcd_map) {
  attn_mfma2_body<HS, SB, PAD>(p, nqb, aligned_dst, xcd_map);
}
// head size 256 (GPT-J, Gemma): 128 accumulator + 64 query registers per lane -> one wave per SIMD with the whole register file,
// one workgroup per CU (two stages of 66 KB)
template <bool SB = false, bool PAD = false>
__global__ __launch_bounds__(256) void attn_mfma2_hs256_kernel(const AttnParams p, const int nqb, const int aligned_dst, const int xcd_map) {
  attn_mfma2_body<256, SB, PAD>(p, nqb, aligned_dst, xcd_map);
}

// the PAGED instantiations (ns_hip_attn_prefill_paged): the same register budgets
template <int HS, bool SB, bool PAD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_mfma2_paged_kernel(const AttnPrefillPagedParams pp, const int nqb, const int aligned_dst,
                                                                                                    const int xcd_map) {
  attn_mfma2_body<HS, SB, PAD, 1, true>(pp, nqb, aligned_dst, xcd_map);
}
// (no head-size-256 form: with the whole register file it still needs 116 .. 196 bytes of scratch per lane — the plan refuses head sizes above 128)

// ---- launch of a plan (ns_attn_plan.cpp): pl.hs_pad, pl.sb and pl.pad are the template arguments -----------------------------------------
hipError_t launch_attn_rows(const AttnPlan& pl, hipStream_t st) {
  const AttnParams& p = pl.sp.a;
  if (pl.path == AP_ROWS64) {
    if (pl.hs_pad == 64)
      hipLaunchKernelGGL(attn_mfma_kernel<64>, pl.grid, pl.block, 0, st, p);
    else
      hipLaunchKernelGGL(attn_mfma_kernel<128>, pl.grid, pl.block, 0, st, p);
    return hipGetLastError();
  }
  auto go = [&](auto kern_c) {  // (kernel_c: the kernel is part of the argument's type, so each has its own LDS limit)
    return launch_lds<decltype(kern_c)::value>(int(pl.lds), pl.grid, pl.block, pl.lds, st, p, pl.nqb, pl.aligned, pl.xcd_map);
  };
  if (pl.path == AP_PIPELINED) return pl.hs_pad == 64 ? go(kernel_c<attn_mfma3_kernel<64>>{}) : go(kernel_c<attn_mfma3_kernel<128>>{});
  auto by_hs = [&](auto sb_c, auto pad_c) {
    constexpr bool SB = decltype(sb_c)::value, PAD = decltype(pad_c)::value;
    if (pl.hs_pad == 256) return go(kernel_c<attn_mfma2_hs256_kernel<SB, PAD>>{});
    return pl.hs_pad == 64 ? go(kernel_c<attn_mfma2_kernel<64, SB, PAD>>{}) : go(kernel_c<attn_mfma2_kernel<128, SB, PAD>>{});
  };
  if (pl.sb) return pl.pad ? by_hs(std::true_type{}, std::true_type{}) : by_hs(std::true_type{}, std::false_type{});
  return pl.pad ? by_hs(std::false_type{}, std::true_type{}) : by_hs(std::false_type{}, std::false_type{});
}
hipError_t launch_attn_prefill_paged(const AttnPrefillPagedPlan& pl, hipStream_t st) {
  auto go = [&](auto kern_c) {
    return launch_lds<decltype(kern_c)::value>(int(pl.lds), pl.grid, pl.block, pl.lds, st, pl.pp, pl.nqb, pl.aligned, pl.xcd_map);
  };
  auto by_hs = [&](auto sb_c, auto pad_c) {
    constexpr bool SB = decltype(sb_c)::value, PAD = decltype(pad_c)::value;
    if (pl.hs_pad != 64 && pl.hs_pad != 128) return hipErrorInvalidValue;  // (no plan names another)
    return pl.hs_pad == 64 ? go(kernel_c<attn_mfma2_paged_kernel<64, SB, PAD>>{}) : go(kernel_c<attn_mfma2_paged_kernel<128, SB, PAD>>{});
  };
  if (pl.sb) return pl.pad ? by_hs(std::true_type{}, std::true_type{}) : by_hs(std::true_type{}, std::false_type{});
  return pl.pad ? by_hs(std::false_type{}, std::true_type{}) : by_hs(std::false_type{}, std::false_type{});
}
void touch_attn_rows_module() { touch_kernel(reinterpret_cast<const void*>(attn_mfma3_kernel<128>)); }

}  // namespace ns
