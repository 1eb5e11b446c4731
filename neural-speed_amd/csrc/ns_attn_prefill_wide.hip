// ns_attn_prefill_wide.hip — prompt-sized query blocks over the fp16 paged pools at head sizes 136 .. 256 (ns_hip_attn_prefill_paged_wide):
// attn_wide_paged_kernel and the launch of its plan (attn_prefill_paged_wide_plan, ns_attn_plan.cpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "ns_attn.h"
#include "ns_launch.h"

namespace ns {

// ============================================================================================================
// attn_wide_paged_kernel — the arithmetic of attn_mfma2_kernel at head size 256 (128 query rows of one (head, request) per workgroup, 32 per wave,
// v_mfma_f32_32x32x16_f16, Q in 64 registers, 128 accumulators, exp2-domain softmax with one lane ^ 32 exchange per tile, lane-local rescale) with
// the 64-key K / V tiles travelling pool -> LDS by DMA (buffer_load ... lds, 16 bytes per lane, 1 KiB per wave-wide request) THROUGH ONE BUFFER
// DESCRIPTOR PER PAGE AND WAVE.  The PAGED instantiation of attn_mfma2_body at this width needs all 512 registers and 116 .. 196 bytes of scratch:
// 64 staging registers carry a tile from global memory to LDS and every 16-byte chunk pays a 64-bit page address with its range check.  Here
// neither exists:
//   split     of a tile's 64 keys wave w moves keys 16 w .. 16 w + 15, K and V alike: an aligned group of 16 — tiles start at multiples of 64 and a
//             page holds 16 keys or more, so the group lies in ONE page and one table entry per wave and tile serves its 16 requests (8 of K: two
//             512-byte rows each; 8 of V: 16 rows x 32 dims each).
//   table     lane l fetches the entry of group l & 3 of tile b + 1 while tile b + 1's requests are issued (a vector load: it retires with them);
//             the wave reads its own by v_readlane.  The key whose entry is read is clamped to the last live one (attn_prefill_tile_key), so no
//             entry at or behind ceil(kv_len / block_keys) is read.
//   rsrc      from the entry the wave builds, in scalar registers, base = pool + id * block_step + ihkv * step_head + (first key's row in the page)
//             * step_sl (64-bit) and num_records = ((live keys of the group under kv_len - 1) * step_sl + head_size) * 2 bytes — 0 for a group at or
//             behind kv_len and for an id outside [0, pool_blocks) (attn_wide_desc, ns_attn.h).
//   lane      offsets are tile-invariant, 16 registers computed once (attn_wide_k_offset / attn_wide_v_offset): the DMA writes lane-linear, so the
//             XOR swizzle of a K row's 16-byte slots and the V image are made by WHICH global 16 bytes a lane asks for.  A key at or behind kv_len
//             lies outside num_records and arrives as zeros; with PAD a chunk at or past head_size asks for kAwNoCell, outside every descriptor:
//             the next head's bytes are never read.  No clamp, no per-row address, no range check on the VALU, no staging register in the loop.
//   V image   [8 column blocks of 32 dims][64 keys][32 dims]: a request (column block u, the wave's 16 keys) is 1 KiB contiguous in LDS AND inside
//             one page, which the 128-row kernels' [16-dim subtile][64 keys] image (32 keys per request) is not on pages of 16.  ds_read_b64_tr_b16
//             reads it as before — a lane's (key, dims) are those of attn_mfma2_body — and the 32 lanes of a half-wave cover 4 keys x 64 bytes =
//             256 contiguous bytes: every bank once, without the 128-byte subtile offset.
//   stages    two of 64 KiB (K 32 KiB | V 32 KiB) = 128 KiB of the CU's 160: one workgroup per CU, one wave per SIMD with the whole register file.
//             64-key tiles: a third stage does not fit beside them, and 32-key tiles (four stages) would halve what a barrier and a softmax
//             exchange are spread over while the per-tile descriptor work stayed — not built.
//   schedule  the requests of tile b + 1 are issued behind K(b) . Q^T; every wave waits for its own (s_waitcnt vmcnt(0): its 16 requests and the
//             table entry are all it has in flight) in front of the tile's one barrier.
// Per-request geometry as in the PAGED body: a query block the request does not have leaves in front of any barrier, a wave without a live row keeps
// every barrier and its share of the requests, rows that see no key are zeros.  No score bias (the plan refuses ALiBi, the tanh cap and a score scale
// that is not positive).
// ============================================================================================================
typedef _Float16 whalf8_t __attribute__((ext_vector_type(8)));
typedef _Float16 whalf4_t __attribute__((ext_vector_type(4)));
typedef float wfloatx4 __attribute__((ext_vector_type(4)));
typedef float wfloatx16 __attribute__((ext_vector_type(16)));
typedef short wshort4_t __attribute__((ext_vector_type(4)));

template <bool PAD>
__global__ __launch_bounds__(256) void attn_wide_paged_kernel(const AttnPrefillPagedParams pp, const int nqb, const int aligned_dst, const int xcd_map) {
  constexpr int HS = 256, NJ = HS / 16, NDT = HS / 32, KROW = HS * 2;
  const AttnParams& p = pp.a;
  extern __shared__ __attribute__((aligned(16))) unsigned char smemw[];  // [2 stages][K 32 KiB | V 32 KiB]
  using LdsPtr [[maybe_unused]] = __attribute__((address_space(3))) unsigned char*;  // (used by the device side only)
  const int tid = threadIdx.x, l = tid & 63, n = l & 31, h = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool causal = (p.flags & NS_ATTN_FLAG_IS_CAUSAL) != 0;
  // workgroup -> (query block, head, request): attn_mfma2_body's order (the query blocks and query heads of a kv head on one XCD; heaviest-first in
  // the first half of the units, lightest-first in the second)
  const unsigned G = unsigned(p.head_num / p.heads_kv), units = gridDim.x / unsigned(nqb);
  unsigned unit = blockIdx.x / unsigned(nqb), ordn = blockIdx.x % unsigned(nqb);
  bool heavy_first = unit < (units + 1) / 2;
  if (xcd_map) {
    const unsigned x = blockIdx.x & 7u, sl = blockIdx.x >> 3;
    const unsigned ul = sl / unsigned(nqb);
    ordn = sl % unsigned(nqb);
    unit = ((ul / G) * 8u + x) * G + ul % G;
    heavy_first = ul < (units / 8u + 1) / 2;
  }
  const int qblk = causal && heavy_first ? nqb - 1 - int(ordn) : int(ordn);
  const int ihn = int(unit) % p.head_num, ibs = int(unit) / p.head_num;
  const int ihkv = ihn / (p.head_num / p.heads_kv);
  const int q_len = attn_block_q_len(pp.q_start, ibs, p.sl_q);
  const int kv_len = attn_prefill_kv_len(pp.kv_lens, ibs, pp.kdelta, p.sl_kv);
  if (qblk * 128 >= q_len) return;  // no row of this query block is a row of the request (workgroup-uniform, in front of any barrier)
  const long long q_base = pp.q_start[ibs];
  const int off = kv_len - q_len;
  const int q0 = qblk * 128 + w * 32;
  const float* qb = p.q + q_base * p.step_q_sl + ihn * p.step_q_head_num;
  float* db = p.dst + q_base * p.step_dst_sl + ihn * p.step_dst_head_num;
  const int hs = PAD ? p.head_size : HS;  // PAD: query dims, K / V chunks and output dims from hs on are zeros / never stored

  whalf8_t qf[NJ];
  wfloatx16 o[NDT];
  float m_run = -INFINITY, l_run = 0.f;  // l_run: this lane's half of the row sum
  {
    const float* qr = qb + (long long)min(q0 + n, q_len - 1) * p.step_q_sl + 8 * h;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const bool in = 16 * j + 8 * h < hs;     // (a chunk the head does not have is loaded from dim 8 h, which it has, and dropped: no branch per load)
      const float* qc = qr + (in ? 16 * j : 0);
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const float x = qc[i];
        qf[j][i] = in ? (_Float16)x : (_Float16)0.f;
      }
    }
#pragma unroll
    for (int dt = 0; dt < NDT; dt++)
#pragma unroll
      for (int i = 0; i < 16; i++) o[dt][i] = 0.f;
  }
  const float sc = p.qk_scale * 1.4426950408889634f;  // scores in the exp2 domain (positive and finite: the plan's rule)
  const int q_last_wg = min(qblk * 128 + 127, q_len - 1);
  const int kv_end = causal ? min(kv_len, q_last_wg + off + 1) : kv_len;  // workgroup-uniform; may be <= 0 (more rows than keys)
  const int visible = min(kv_len, causal ? min(q0 + n, q_len - 1) + off + 1 : kv_len);
  const int vis_first = min(kv_len, causal ? q0 + off + 1 : kv_len);
  const int vis_last = min(kv_len, causal ? min(q0 + 31, q_len - 1) + off + 1 : kv_len);
  const bool wave_live = q0 < q_len;

  // ---- tile requests: tile-invariant lane offsets, one descriptor pair per wave and tile ----
  uint32_t kvoff[kAwReq], vvoff[kAwReq];
#pragma unroll
  for (int u = 0; u < kAwReq; u++) {
    kvoff[u] = attn_wide_k_offset(u, l, p.step_k_sl, hs);
    vvoff[u] = attn_wide_v_offset(u, l, p.step_v_sl, hs);
  }
  const int* trow = pp.pg.table + (long long)ibs * pp.pg.table_stride;
  auto fetch_id = [&](int pos0) { return trow[attn_wide_table_slot(pp.pg, pos0, l & 3, kv_len)]; };  // (kv_len >= 1 wherever a tile is fetched: nb > 0)
  auto rsrc_of = [](const _Float16* pool, const AttnWideDesc& d) {
    const uint64_t v = reinterpret_cast<uint64_t>(pool + d.base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(v)), hi = __builtin_amdgcn_readfirstlane(uint32_t(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<_Float16*>((uint64_t(hi) << 32) | lo), 0, __builtin_amdgcn_readfirstlane(d.bytes), 0x00020000);
  };
  int idv = 0;  // lane l: the table entry of group l & 3 of the tile the NEXT issue requests
  auto issue = [&](int t, int buf) {
    const int pos0 = t * kA2KB;
    const int id = __builtin_amdgcn_readlane(idv, w);
    const __amdgpu_buffer_rsrc_t rk = rsrc_of(p.k, attn_wide_desc(pp.pg, id, pos0, w, kv_len, ihkv, p.step_k_sl, p.step_k_head_num, hs));
    const __amdgpu_buffer_rsrc_t rv = rsrc_of(p.v, attn_wide_desc(pp.pg, id, pos0, w, kv_len, ihkv, p.step_v_sl, p.step_v_head_num, hs));
    idv = fetch_id(pos0 + kA2KB);  // (clamped to the last live key: a live entry also behind the last tile)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int u = 0; u < kAwReq; u++)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, reinterpret_cast<__attribute__((address_space(3))) void*>((LdsPtr)(smemw) + buf * kAwStage + attn_wide_k_lds(w, u)),
                                               16, kvoff[u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < kAwReq; u++)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, reinterpret_cast<__attribute__((address_space(3))) void*>((LdsPtr)(smemw) + buf * kAwStage + attn_wide_v_lds(w, u)),
                                               16, vvoff[u], 0, 0, 0);
#else
    (void)rk, (void)rv, (void)buf;
#endif
  };
  // operand addresses inside a stage
  const int swz_n = n & 15;
  const int k_rd = n * KROW;                                                                          // + 32 T rows, slot (2 j + h) ^ swizzle
  const int v_rd = kAwKTile + (4 * h + ((l & 15) >> 2)) * 64 + ((l >> 4) & 1) * 32 + (l & 3) * 8;  // + column block dt * 4 KiB, + 16-key step ts * 1 KiB, + 8 keys * 64

  const int nb = (kv_end + kA2KB - 1) / kA2KB;
  if (nb > 0) {
    idv = fetch_id(0);
    issue(0, 0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int b = 0; b < nb; b++) {
    const int pos0 = b * kA2KB;
    const bool more = b + 1 < nb;
    const unsigned char* sb = smemw + (b & 1) * kAwStage;
    if (wave_live && pos0 < vis_last) {
      // S^T = K(b) . Q^T: operands travel LDS -> registers one group of four MFMAs ahead of their use (two register sets, fenced)
      wfloatx16 sv[2];
#pragma unroll
      for (int T = 0; T < 2; T++)
#pragma unroll
        for (int i = 0; i < 16; i++) sv[T][i] = 0.f;
      {
        constexpr int CPT = NJ / 4, NCK = 2 * CPT;
        whalf8_t kf[2][4];
        auto ldk = [&](int c, whalf8_t(&dst)[4]) {
          const int T = c / CPT, j0 = (c % CPT) * 4;
#pragma unroll
          for (int u = 0; u < 4; u++) dst[u] = *reinterpret_cast<const whalf8_t*>(sb + k_rd + 32 * T * KROW + (((2 * (j0 + u) + h) ^ swz_n) << 4));
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
      }
      if (more) issue(b + 1, (b + 1) & 1);
      // softmax in the exp2 domain on the raw scores: p = exp2(s sc - m sc); the running maximum is kept unscaled
      if (pos0 + kA2KB > vis_first) {  // wave-uniform: only tiles on the diagonal / past the last key are masked
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
      const float neg_m = m_new == -INFINITY ? 0.f : -m_new * sc;  // nothing visible yet: every exp2 below is exp2(-inf) = 0
      const float alpha = __builtin_amdgcn_exp2f(fmaf(m_run, sc, neg_m));
      float ps = 0.f;
      whalf8_t pf[4];  // (T, s) -> 2 T + s
#pragma unroll
      for (int e = 0; e < 32; e++) {
        const float pe = __builtin_amdgcn_exp2f(fmaf(sv[e >> 4][e & 15], sc, neg_m));
        ps += pe;
        pf[e >> 3][e & 7] = (_Float16)pe;
      }
      l_run = l_run * alpha + ps;
      m_run = m_new;
      if (__any(alpha != 1.f)) {
#pragma unroll
        for (int dt = 0; dt < NDT; dt++)
#pragma unroll
          for (int i = 0; i < 16; i++) o[dt][i] *= alpha;
      }
      // O^T += V(b)^T . P^T
      {
        whalf8_t vf[2][4];
        auto ldv = [&](int dt, whalf8_t(&dst)[4]) {
#pragma unroll
          for (int ts = 0; ts < 4; ts++) {
            const unsigned char* va = sb + v_rd + dt * 4096 + ts * 1024;
            const wshort4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wshort4_t __attribute__((address_space(3)))*)(va));
            const wshort4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wshort4_t __attribute__((address_space(3)))*)(va + 8 * 64));
            dst[ts] = __builtin_bit_cast(whalf8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
          }
        };
        ldv(0, vf[0]);
#pragma unroll
        for (int dt = 0; dt < NDT; dt++) {
          if (dt + 1 < NDT) ldv(dt + 1, vf[(dt + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int ts = 0; ts < 4; ts++) o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[dt & 1][ts], pf[ts], o[dt], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    } else if (more) {
      issue(b + 1, (b + 1) & 1);
    }
    // this wave's requests have landed; every wave is done with tile b's stage
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  l_run += __shfl_xor(l_run, 32, 64);
  const float inv = l_run > 0.f ? p.out_scale / l_run : 0.f;
  const int row = q0 + n;
  if (row < q_len) {
    float* dr = db + (long long)row * p.step_dst_sl;
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) {
#pragma unroll
      for (int bq = 0; bq < 4; bq++) {
        const int d = 32 * dt + 8 * bq + 4 * h;
        if (PAD && d >= hs) continue;
        const wfloatx4 y = wfloatx4{o[dt][4 * bq] * inv, o[dt][4 * bq + 1] * inv, o[dt][4 * bq + 2] * inv, o[dt][4 * bq + 3] * inv};
        if (aligned_dst) {
          *reinterpret_cast<wfloatx4*>(dr + d) = y;
          if (p.dst16) *reinterpret_cast<whalf4_t*>(p.dst16 + (dr - p.dst) + d) = whalf4_t{(_Float16)y[0], (_Float16)y[1], (_Float16)y[2], (_Float16)y[3]};
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

hipError_t launch_attn_prefill_paged_wide(const AttnPrefillWidePlan& pl, hipStream_t st) {
  if (!pl.ok) return hipErrorInvalidValue;
  if (pl.pad) return launch_lds<attn_wide_paged_kernel<true>>(int(pl.lds), pl.grid, pl.block, pl.lds, st, pl.pp, pl.nqb, pl.aligned, pl.xcd_map);
  return launch_lds<attn_wide_paged_kernel<false>>(int(pl.lds), pl.grid, pl.block, pl.lds, st, pl.pp, pl.nqb, pl.aligned, pl.xcd_map);
}

}  // namespace ns
