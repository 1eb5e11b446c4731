// ns_attn_decode_f8.hip — decode over an FP8 (E4M3) paged KV cache: the kernels of ns_hip_attn_decode_paged_f8 and the launch of its plan
// (attn_decode_paged_f8_plan, ns_attn_plan.cpp).  The pools are those of ns_hip_attn_decode_paged with one byte per element (ns_attn.h, "an FP8 paged
// cache"); Q, the output, the partials and the merge are fp32 as ever, so attn_split_finish and attn_merge_kernel<true> serve unchanged.
//
// attn_stream8_kernel (head sizes 48 .. 128): attn_stream_kernel's ring with HALF the requests per key.  A wave-wide buffer_load ... lds is 1 KiB, 16
//   bytes per lane, whatever the element: with byte elements a key row is RL = 8 request lanes (head sizes 80 .. 128) or 4 (48 / 64), so one request
//   carries 8 or 16 CONSECUTIVE keys where the fp16 kernel's carries 4 or 8.  The image in LDS is lane-linear: [keys of the request][RL * 16 bytes].
//   The arithmetic does not change: LPK = 2 RL lanes per key with 8 dims each, so a request is TWO sub-steps of the fp16 kernel's form — half h of a
//   slot image (bytes h * 512 ..) holds keys KPW * h .. KPW * h + KPW - 1 of the request in exactly the lane order of that form, and lane l reads its 8
//   bytes at h * 512 + l * 8 (ds_read_b64, lane-linear, no bank conflict).  Ring geometry, slot size, the query rows requested first and the counted
//   vmcnt (two requests per slot) are the fp16 kernel's; a softmax update covers U sub-steps = U / 2 slots, the same number of keys, so the fp16
//   plan's ranges apply; a workgroup's ring holds 8 slots x 4 waves x 2 KPW keys: 256 keys in flight at head sizes 80 .. 128 (fp16: 128), 512 below.
//   Paging as in the PAGED fp16 form: a request's 8 or 16 consecutive keys lie in at most two blocks, both table entries are wave-uniform scalar
//   loads, each lane picks its block and forms its byte offset into ONE descriptor over the pool; pool_bytes — outside it — stands for "no access".
// attn_split8_kernel (every other head size that is a multiple of 16, and pools the byte rule keeps from the ring): attn_split_kernel's PAGED shape
//   with 8 (16) byte loads per lane through 64-bit addresses.
// Both: codes are selected to zero for masked keys and lanes past the head size BEFORE they are decoded (a NaN code there must not reach a sum),
// decoded exactly by CDNA4's packed conversion (0x7f / 0xff give NaN), then the fp16 kernels' update and finish.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ns_attn.h"
#include "ns_attn_onerow.h"
#include "ns_launch.h"

namespace ns {

typedef uint32_t u2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u4_t __attribute__((ext_vector_type(4)));

// four E4M3 codes of a dword -> four fp32 values, exact (v_cvt_pk_f32_fp8: the low or the high pair of codes)
__device__ __forceinline__ void e4m3x4_to_f32(uint32_t w, float* f) {
  typedef float f2_t __attribute__((ext_vector_type(2)));
  const f2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(int(w), false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(int(w), true);
  f[0] = lo.x, f[1] = lo.y, f[2] = hi.x, f[3] = hi.y;
}

// One softmax update of head g over U keys per lane (attn_split_kernel's, operation for operation): kf / vf are the lane's DPL dims of its U keys, j[u]
// the keys, reduced over the LPK lanes of a key.
template <int U, int DPL, int LPK>
__device__ __forceinline__ void attn_update8(const float (&q)[DPL], float (&acc)[DPL], float& m, float& lsum, float slope, const float (&kf)[U][DPL],
                                             const float (&vf)[U][DPL], const int (&j)[U], int j1, bool tanh30) {
  float s[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    float t2 = 0.f;
#pragma unroll
    for (int e = 0; e < DPL; e++) t2 += q[e] * kf[u][e];
    s[u] = t2;
  }
#pragma unroll
  for (int off = LPK / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int u = 0; u < U; u++) s[u] += __shfl_xor(s[u], off, 64);
  }
  float m_new = m;
#pragma unroll
  for (int u = 0; u < U; u++) {
    if (tanh30) s[u] = 30.f * tanhf(s[u] * (1.f / 30.f));
    s[u] += float(j[u]) * slope;
    if (j[u] >= j1) s[u] = -INFINITY;
    m_new = fmaxf(m_new, s[u]);
  }
  // a lane group whose keys of this batch are all past the end keeps m = -inf: then m_new = -inf and exp(-inf - -inf) would be NaN
  const float corr = m_new == -INFINITY ? 1.f : expf(m - m_new);
  float pj[U], psum = 0.f;
#pragma unroll
  for (int u = 0; u < U; u++) {
    pj[u] = m_new == -INFINITY ? 0.f : expf(s[u] - m_new);
    psum += pj[u];
  }
  lsum = lsum * corr + psum;
#pragma unroll
  for (int e = 0; e < DPL; e++) {
    float a2 = acc[e] * corr;
#pragma unroll
    for (int u = 0; u < U; u++) a2 += pj[u] * vf[u][e];
    acc[e] = a2;
  }
  m = m_new;
}

__device__ __forceinline__ float alibi_slope(const AttnParams& p, int ihn) {
  const int gh = ihn + p.alibi_head_off;
  return gh < p.alibi_log2_floor ? powf(p.alibi_m0, float(gh + 1)) : powf(p.alibi_m1, float(2 * (gh - p.alibi_log2_floor) + 1));
}

// ---------------------------------------------------------------------------------------------------------------
// register form
// ---------------------------------------------------------------------------------------------------------------
template <int G, int DPL>  // G query heads per kv head; DPL head dims (bytes) per lane: 8 (head_size <= 128) or 16 (<= 256)
__global__ __launch_bounds__(kAttnThreads) void attn_split8_kernel(const AttnPagedParams kp) {
  const AttnSplitParams& sp = kp.sp;
  const AttnPage& pg = kp.pg;
  const AttnParams& p = sp.a;
  __shared__ float ml_s[4][G][2];
  extern __shared__ float acc_s[];  // [4 waves][G][16 * DPL]
  const int split = sp.heads_first ? blockIdx.y : blockIdx.x;
  const int by = sp.heads_first ? blockIdx.x : blockIdx.y;
  const int chunk = by % sp.chunks, ykv = by / sp.chunks;
  const int ihkv = ykv % p.heads_kv, i = ykv / p.heads_kv, ibs = blockIdx.z;
  auto head_of = [&](int g) { return ihkv * sp.g_full + min(chunk * G + g, sp.g_full - 1); };
  const int t = threadIdx.x, l = t & 63;
  const int kg = t >> 4;  // key group 0..15
  const int dl = l & 15;  // dim lane
  const int hs = p.head_size;
  const bool alibi = (p.flags & NS_ATTN_FLAG_IS_ALIBI8) != 0;
  const bool tanh30 = (p.flags & NS_ATTN_FLAG_IS_TANH30) != 0;
  const int sl_kv = attn_live_kv<true>(sp, ibs), live = attn_live_splits(sp, sl_kv);
  if (sl_kv == 0) {  // an idle slot
    if (split == 0) attn_zero_rows<G>(sp, chunk, ihkv, i, ibs);
    return;
  }
  if (split >= live) return;
  const int kps = attn_live_kps(sp, sl_kv);
  const int j0 = split * kps, j1 = min(sl_kv, j0 + kps);  // (one query row, the last of its context: causal masks nothing)
  const int d0 = dl * DPL;
  const bool dact = d0 < hs;
  const unsigned char* kb = reinterpret_cast<const unsigned char*>(p.k) + ihkv * p.step_k_head_num + d0;
  const unsigned char* vb = reinterpret_cast<const unsigned char*>(p.v) + ihkv * p.step_v_head_num + d0;

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
    slope[g] = alibi ? alibi_slope(p, ihn) : 0.f;
  }
  constexpr int U = G * DPL <= 16 ? 4 : (G * DPL <= 64 ? 2 : 1);  // attn_split_kernel's register budget
  typedef std::conditional_t<DPL == 8, u2_t, u4_t> Codes;
  for (int jb = j0 + kg; jb < j1; jb += 16 * U) {
    Codes kc[U], vc[U];
#pragma unroll
    for (int u = 0; u < U; u++) {  // the U keys' rows are requested together; -1: no access, the key reads as zeros
      const int j = jb + 16 * u;
      long long ck = -1, cv = -1;
      if (dact && j < j1) ck = attn_page_cell(pg, ibs, j, p.step_k_sl), cv = attn_page_cell(pg, ibs, j, p.step_v_sl);
      kc[u] = Codes(0u), vc[u] = Codes(0u);
      if (ck >= 0 && cv >= 0) {
        kc[u] = __builtin_nontemporal_load(reinterpret_cast<const Codes*>(kb + ck));
        vc[u] = __builtin_nontemporal_load(reinterpret_cast<const Codes*>(vb + cv));
      }
    }
    float kf[U][DPL], vf[U][DPL];
    int jj[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      jj[u] = jb + 16 * u;
#pragma unroll
      for (int c = 0; c < DPL / 4; c++) {
        e4m3x4_to_f32(kc[u][c], &kf[u][4 * c]);
        e4m3x4_to_f32(vc[u][c], &vf[u][4 * c]);
      }
    }
#pragma unroll
    for (int g = 0; g < G; g++) attn_update8<U, DPL, 16>(q[g], acc[g], m[g], lsum[g], slope[g], kf, vf, jj, j1, tanh30);
  }
  attn_split_finish<G, DPL>(sp, acc, m, lsum, acc_s, ml_s, split, chunk, ihkv, i, ibs, live);
}

// ---------------------------------------------------------------------------------------------------------------
// ring form
// ---------------------------------------------------------------------------------------------------------------
template <int G, int LPK>  // LPK arithmetic lanes per key: 16 (head sizes 80 .. 128, 8 keys per request) or 8 (48 / 64, 16 keys per request)
__global__ __launch_bounds__(kAttnThreads) void attn_stream8_kernel(const AttnPagedParams kp) {
  const AttnSplitParams& sp = kp.sp;
  const AttnPage& pg = kp.pg;
  constexpr int DPL = 8;
  constexpr int RL = LPK / 2;        // request lanes per key row: 16 bytes each
  constexpr int KPW = 64 / LPK;      // keys per wave and sub-step
  constexpr int KPR = 2 * KPW;       // keys per wave and request (slot)
  constexpr int KPS = 4 * KPR;       // keys per workgroup and slot
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
  const int hs = p.head_size;
  const bool alibi = (p.flags & NS_ATTN_FLAG_IS_ALIBI8) != 0;
  const bool tanh30 = (p.flags & NS_ATTN_FLAG_IS_TANH30) != 0;
  const int sl_kv = attn_live_kv<true>(sp, ibs), live = attn_live_splits(sp, sl_kv);
  if (sl_kv == 0) {  // an idle slot
    if (split == 0) attn_zero_rows<G>(sp, chunk, ihkv, i, ibs);
    return;
  }
  if (split >= live) return;
  const int kps = attn_live_kps(sp, sl_kv);
  const int j0 = split * kps, j1 = min(sl_kv, j0 + kps);
  const int d0 = (l & (LPK - 1)) * DPL;  // the lane's dims of the arithmetic
  const bool dact = d0 < hs;
  const int r0 = (l & (RL - 1)) * 16;    // ... and of its request; head sizes are multiples of 16, so a lane requests iff both its arithmetic lanes are live
  [[maybe_unused]] const bool ract = r0 < hs;
  constexpr int U = G * DPL <= 16 ? 4 : 2;  // sub-steps per softmax update: attn_stream_kernel's rule
  constexpr int UR = U / 2;                 // ... = slots per update
  static_assert(kAsSteps % UR == 0 && kAsSteps == 8, "a batch never wraps inside the ring; the vmcnt cases below");
  const int nreq = j1 > j0 ? (((j1 - j0 + KPS - 1) / KPS) + UR - 1) / UR * UR : 0;  // whole batches: slots past the end fetch nothing

  // ---- 0. the table entries of the first ring (scalar loads) and the query rows (older than the stream) — as attn_stream_kernel, which says why ----
  const int tshift = pg.block_shift;
  const int* trow = pg.table + (long long)ibs * pg.table_stride;
  auto fetch_ids = [&](int s, int& ba, int& bb) {
    const int a = j0 + KPS * s + KPR * w;
    const int ea = min(a >> tshift, pg.table_stride - 1), eb = min((a + KPR - 1) >> tshift, pg.table_stride - 1);
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
#pragma unroll
  for (int s = 0; s < kAsSteps; s++) fetch_ids(s, ida[s], idb[s]);
  typedef float f4_t __attribute__((ext_vector_type(4)));
  f4_t qa[G], qb[G];
#pragma unroll
  for (int g = 0; g < G; g++) {
    const float* qp = p.q + ibs * p.step_q_bs + head_of(g) * p.step_q_head_num + i * p.step_q_sl + (dact ? d0 : 0);
    asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:16" : "=&v"(qa[g]), "=&v"(qb[g]) : "v"(qp) : "memory");
  }
  __builtin_amdgcn_sched_barrier(0);
  // ---- 1. the whole range (up to the ring's depth) is requested before anything else is touched ----
  // (one descriptor spans each pool: attn_decode_paged_f8_plan gives this kernel only pools of less than 4 GiB, attn_page_in32_f8)
  const uint32_t pool_bytes = uint32_t(size_t(pg.pool_blocks) * size_t(pg.block_step));
  auto uniform_ptr = [](const void* ptr) {
    const uint64_t v = reinterpret_cast<uint64_t>(ptr);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(v)), hi = __builtin_amdgcn_readfirstlane(uint32_t(v >> 32));
    return reinterpret_cast<unsigned char*>((uint64_t(hi) << 32) | lo);
  };
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(p.k), 0, __builtin_amdgcn_readfirstlane(pool_bytes), 0x00020000);
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(p.v), 0, __builtin_amdgcn_readfirstlane(pool_bytes), 0x00020000);
  const LdsPtr ring = (LdsPtr)(ring_s) + w * (kAsSteps * 2048);
  // slot s with its two table entries: the lane's key of the request, its block of the two, its cell through attn_page_at
  auto issue = [&](int s, int ba, int bb) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int a = j0 + KPS * s + KPR * w, key = a + l / RL;
    const int blk = (key >> tshift) == (a >> tshift) ? ba : bb;
    const long long ck = attn_page_at(pg, blk, key, p.step_k_sl), cv = attn_page_at(pg, blk, key, p.step_v_sl);
    const bool on = key < j1 && ck >= 0;
    const uint32_t ko = on ? uint32_t(ck + ihkv * p.step_k_head_num + r0) : pool_bytes;
    const uint32_t vo = on ? uint32_t(cv + ihkv * p.step_v_head_num + r0) : pool_bytes;
    const LdsPtr dst = ring + (s & (kAsSteps - 1)) * 2048;
    if (ract) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, reinterpret_cast<__attribute__((address_space(3))) void*>(dst), 16, ko, 0, 0, 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, reinterpret_cast<__attribute__((address_space(3))) void*>(dst + 1024), 16, vo, 0, 0, 2);
    }
#endif
  };
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int s = 0; s < kAsSteps; s++) asm volatile("" : "+s"(ida[s]), "+s"(idb[s]));  // (uses stay behind the wait)
#pragma unroll
  for (int s = 0; s < kAsSteps; s++)
    if (s < nreq) issue(s, ida[s], idb[s]);
  __builtin_amdgcn_sched_barrier(0);

  // ---- 2. the query rows' first use: their wait is counted, two younger requests per slot stay in flight ----
  switch (min(nreq, kAsSteps)) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
  }
  float q[G][DPL], acc[G][DPL], m[G], lsum[G], slope[G];
#pragma unroll
  for (int g = 0; g < G; g++) {
    asm volatile("" : "+v"(qa[g]), "+v"(qb[g]));  // (uses of the rows stay behind the wait)
#pragma unroll
    for (int e = 0; e < DPL; e++) {
      q[g][e] = dact ? (e < 4 ? qa[g][e & 3] : qb[g][e & 3]) * p.qk_scale : 0.f;
      acc[g][e] = 0.f;
    }
    m[g] = -INFINITY;
    lsum[g] = 0.f;
    slope[g] = alibi ? alibi_slope(p, head_of(g)) : 0.f;
  }

  const uint32_t lane_lds = uint32_t(reinterpret_cast<uintptr_t>(ring)) + uint32_t(l) * 8u;
  // at most `younger` SLOTS requested after the batch about to be read are still in flight (two requests per slot)
  auto wait_slots = [&](int younger) {
    switch (younger) {
      case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
      case 1: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
      case 2: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
      case 3: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
      case 4: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
      case 5: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
      case 6: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
    }
  };
  for (int s0 = 0; s0 < nreq; s0 += UR) {
    int ra[UR], rb[UR];  // the table entries of the slots this batch's slots are refilled with, requested in front of the batch's own wait
#pragma unroll
    for (int r = 0; r < UR; r++) fetch_ids(s0 + kAsSteps + r, ra[r], rb[r]);
    wait_slots(min(nreq - s0 - UR, kAsSteps - UR));
    u2_t kr[U], vr[U];  // sub-step u = 2 r + h: half h of slot r
#pragma unroll
    for (int r = 0; r < UR; r++) {
      const uint32_t a = lane_lds + uint32_t((s0 + r) & (kAsSteps - 1)) * 2048u;
      asm volatile("ds_read_b64 %0, %4\n\tds_read_b64 %1, %4 offset:512\n\tds_read_b64 %2, %4 offset:1024\n\tds_read_b64 %3, %4 offset:1536"
                   : "=&v"(kr[2 * r]), "=&v"(kr[2 * r + 1]), "=&v"(vr[2 * r]), "=&v"(vr[2 * r + 1])
                   : "v"(a)
                   : "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int u = 0; u < U; u++) asm volatile("" : "+v"(kr[u]), "+v"(vr[u]));  // (uses stay behind the wait)
    __builtin_amdgcn_sched_barrier(0);
    // the slots are free: the slots one ring ahead are requested before this batch is multiplied
#pragma unroll
    for (int r = 0; r < UR; r++) asm volatile("" : "+s"(ra[r]), "+s"(rb[r]));  // (behind the lgkmcnt(0) above: the entries have arrived)
#pragma unroll
    for (int r = 0; r < UR; r++)
      if (s0 + kAsSteps + r < nreq) issue(s0 + kAsSteps + r, ra[r], rb[r]);
    __builtin_amdgcn_sched_barrier(0);
    // keys past the range's end and lanes past the head size count as zeros: selected, never multiplied (what lies there may be a NaN code)
    float kf[U][DPL], vf[U][DPL];
    int jj[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      jj[u] = j0 + KPS * (s0 + u / 2) + KPR * w + KPW * (u & 1) + l / LPK;
      const bool on = dact && jj[u] < j1;
      const u2_t zero = {0u, 0u};
      const u2_t kc = on ? kr[u] : zero, vc = on ? vr[u] : zero;
      e4m3x4_to_f32(kc.x, &kf[u][0]), e4m3x4_to_f32(kc.y, &kf[u][4]);
      e4m3x4_to_f32(vc.x, &vf[u][0]), e4m3x4_to_f32(vc.y, &vf[u][4]);
    }
#pragma unroll
    for (int g = 0; g < G; g++) attn_update8<U, DPL, LPK>(q[g], acc[g], m[g], lsum[g], slope[g], kf, vf, jj, j1, tanh30);
  }
  __syncthreads();  // every wave has left its ring: its first bytes become attn_split_finish's acc_s
  attn_split_finish<G, DPL, LPK>(sp, acc, m, lsum, reinterpret_cast<float*>(ring_s), ml_s, split, chunk, ihkv, i, ibs, live);
}

// ---- launch of a plan (attn_decode_paged_f8_plan) ---------------------------------------------------------------------------------------------------
template <int G>
static hipError_t launch_f8_g(const AttnPlan& pl, const AttnSplitParams& sp, hipStream_t st) {
  const AttnPagedParams pp = {sp, pl.page};
  if (pl.path == AP_RING)
    return pl.lpk == 16 ? launch_lds<attn_stream8_kernel<G, 16>>(int(kAsLdsBytes), pl.grid, pl.block, pl.lds, st, pp)
                        : launch_lds<attn_stream8_kernel<G, 8>>(int(kAsLdsBytes), pl.grid, pl.block, pl.lds, st, pp);
  if (pl.dpl == 8) {
    hipLaunchKernelGGL((attn_split8_kernel<G, 8>), pl.grid, pl.block, pl.lds, st, pp);
  } else {
    hipLaunchKernelGGL((attn_split8_kernel<G, 16>), pl.grid, pl.block, pl.lds, st, pp);
  }
  return hipGetLastError();
}
// ws: the partials (pl.partial_bytes); tickets: the stream's ticket buffer when the plan wants one, nullptr = the merge launch
hipError_t launch_attn_onerow_f8(const AttnPlan& pl, float* ws, uint32_t* tickets, hipStream_t st) {
  if (!pl.f8 || !pl.paged || !pl.rows || (pl.path != AP_RING && pl.path != AP_SPLIT_REGS)) return hipErrorInvalidValue;
  AttnSplitParams sp = pl.sp;
  sp.ws = ws, sp.tickets = tickets;
  hipError_t e = pl.G == 1 ? launch_f8_g<1>(pl, sp, st) : pl.G == 2 ? launch_f8_g<2>(pl, sp, st) : pl.G == 4 ? launch_f8_g<4>(pl, sp, st) : launch_f8_g<8>(pl, sp, st);
  if (e != hipSuccess) return e;
  if (sp.nsplit > 1 && !sp.tickets) e = launch_attn_merge(sp, pl.grid.z, st, true);  // attn_merge_kernel<true>: the partials do not know the cache's type
  return e;
}

void touch_attn_f8_module() { touch_kernel(reinterpret_cast<const void*>(attn_split8_kernel<1, 8>)); }

}  // namespace ns
