// ns_attn_prefill_wide_f8.hip — prompt-sized query blocks over the FP8 (E4M3) paged pools at head sizes 144 .. 256
// (ns_hip_attn_prefill_paged_wide_f8): attn_wide_paged8_kernel and the launch of its plan (attn_prefill_paged_wide_f8_plan, ns_attn_plan.cpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "ns_attn.h"
#include "ns_launch.h"

namespace ns {

// ============================================================================================================
// attn_wide_paged8_kernel — attn_wide_paged_kernel (ns_attn_prefill_wide.hip) over pools of E4M3 codes.  FROM THE LDS IMAGE ON it is that kernel,
// operation for operation: 128 packed query rows per workgroup, 32 per wave, Q in 64 registers, S^T = K . Q^T and O^T += V^T . P^T on
// v_mfma_f32_32x32x16_f16 with operand reads one group of four MFMAs ahead, ds_read_b64_tr_b16 on the [8 column blocks][64 keys][32 dims] V image,
// the XOR-swizzled K image, the exp2-domain softmax with its one lane ^ 32 exchange and the skipped rescale, the same workgroup order and final
// division.  The decode is exact (every E4M3 value is an fp16 value), so the stage holds, byte for byte, what the fp16 kernel's DMA would have put
// there from fp16 pools of the decoded values, and the output holds that kernel's bits.
// New is the way from the pool to the image — the fp16 kernel's DMA has no register between memory and LDS in which a code could be decoded:
//   split     as there: wave w moves keys 16 w .. 16 w + 15 of a tile, K and V alike, through ONE table entry and one buffer descriptor pair per wave
//             and tile (attn_wide8_desc: attn_wide_desc in bytes), the entry fetched one tile ahead and read by v_readlane.
//   requests  a lane's 16 bytes are 16 dims of one key row; a wave's share is 4 requests of K (four 256-byte rows each) and 4 of V (16 rows x 64
//             bytes each) where the fp16 kernel issues 8 + 8.  A key at or behind kv_len, an id outside [0, pool_blocks) and (PAD) a column at or past
//             head_size lie outside num_records and arrive as zero BYTES; code 0x00 is +0.0, so no NaN code behind a live length is ever decoded and
//             nothing is selected.  8 tile-invariant lane offsets (attn_wide8_k_offset / attn_wide8_v_offset).
//   registers plain buffer_load_dwordx4 into 32 staging registers per lane, issued behind K(b) . Q^T where the fp16 kernel issues its DMA, consumed in
//             front of the tile's one barrier.  The compiler knows which registers a vmcnt wait guards, so the loads of tile b + 1 stay in flight
//             through the softmax and the whole of P . V: the wait the fp16 kernel carries in front of P . V does not exist here.
//   decode    once per workgroup: each lane turns its 8 x 16 codes into fp16 with v_cvt_scalef32_pk_f16_fp8 at scale 1.0 (park8's conversion,
//             ns_attn_prefill.hip) and writes them with 16-byte LDS stores into stage (b + 1) & 1 — free since the barrier that ended tile b - 1.
//             K: fp16 chunks c = 2 col, c + 1 of its row to slots c ^ swizzle, (c + 1) ^ swizzle; V: 32 contiguous bytes of its key's 64-byte row
//             in column block col / 2 (attn_wide8_k_lds / attn_wide8_v_lds).
// ============================================================================================================
typedef _Float16 w8half8_t __attribute__((ext_vector_type(8)));
typedef _Float16 w8half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 w8half2_t __attribute__((ext_vector_type(2)));
typedef float w8floatx4 __attribute__((ext_vector_type(4)));
typedef float w8floatx16 __attribute__((ext_vector_type(16)));
typedef short w8short4_t __attribute__((ext_vector_type(4)));
typedef uint32_t w8uint4_t __attribute__((ext_vector_type(4)));

// two dwords of codes -> the 8 fp16 values they name, in order
__device__ __forceinline__ w8half8_t wide8_decode(uint32_t w0, uint32_t w1) {
#ifndef NS_AW8_NODECODE
  const w8half2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true);
  const w8half2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true);
  return w8half8_t{a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
#else  // (scripts/attn_prefill_paged_wide_f8_bench.py's ablation: the loads and the stores without the conversion — wrong results by construction)
  return __builtin_bit_cast(w8half8_t, w8uint4_t{w0, w1, w0, w1});
#endif
}

template <bool PAD>
__global__ __launch_bounds__(256) void attn_wide_paged8_kernel(const AttnPrefillPagedParams pp, const int nqb, const int aligned_dst, const int xcd_map) {
  constexpr int HS = 256, NJ = HS / 16, NDT = HS / 32, KROW = HS * 2;
  const AttnParams& p = pp.a;
  extern __shared__ __attribute__((aligned(16))) unsigned char smemw8[];  // [2 stages][K 32 KiB | V 32 KiB]: the fp16 kernel's image
  const int tid = threadIdx.x, l = tid & 63, n = l & 31, h = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool causal = (p.flags & NS_ATTN_FLAG_IS_CAUSAL) != 0;
  // workgroup -> (query block, head, request): attn_wide_paged_kernel's order
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
  const int hs = PAD ? p.head_size : HS;  // PAD: query dims, K / V columns and output dims from hs on are zeros / never stored

  w8half8_t qf[NJ];
  w8floatx16 o[NDT];
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

  // ---- tile requests: tile-invariant lane offsets and LDS slots, one descriptor pair per wave and tile ----
  uint32_t kvoff[kAw8Req], vvoff[kAw8Req];
#pragma unroll
  for (int u = 0; u < kAw8Req; u++) {
    kvoff[u] = attn_wide8_k_offset(u, l, p.step_k_sl, hs);
    vvoff[u] = attn_wide8_v_offset(u, l, p.step_v_sl, hs);
  }
  const unsigned char* poolk = reinterpret_cast<const unsigned char*>(p.k);  // (bytes behind the fp16 pointer type)
  const unsigned char* poolv = reinterpret_cast<const unsigned char*>(p.v);
  const int* trow = pp.pg.table + (long long)ibs * pp.pg.table_stride;
  auto fetch_id = [&](int pos0) { return trow[attn_wide_table_slot(pp.pg, pos0, l & 3, kv_len)]; };  // (kv_len >= 1 wherever a tile is fetched: nb > 0)
  auto rsrc_of = [](const unsigned char* pool, const AttnWideDesc& d) {
    const uint64_t v = reinterpret_cast<uint64_t>(pool + d.base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(v)), hi = __builtin_amdgcn_readfirstlane(uint32_t(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<unsigned char*>((uint64_t(hi) << 32) | lo), 0, __builtin_amdgcn_readfirstlane(d.bytes), 0x00020000);
  };
  int idv = 0;                    // lane l: the table entry of group l & 3 of the tile the NEXT issue requests
  w8uint4_t stg[2 * kAw8Req];     // the codes of one tile on their way: K's requests, then V's
  auto issue = [&](int t) {
    const int pos0 = t * kA2KB;
    const int id = __builtin_amdgcn_readlane(idv, w);
    const __amdgpu_buffer_rsrc_t rk = rsrc_of(poolk, attn_wide8_desc(pp.pg, id, pos0, w, kv_len, ihkv, p.step_k_sl, p.step_k_head_num, hs));
    const __amdgpu_buffer_rsrc_t rv = rsrc_of(poolv, attn_wide8_desc(pp.pg, id, pos0, w, kv_len, ihkv, p.step_v_sl, p.step_v_head_num, hs));
    idv = fetch_id(pos0 + kA2KB);  // (clamped to the last live key: a live entry also behind the last tile)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int u = 0; u < kAw8Req; u++) stg[u] = __builtin_amdgcn_raw_buffer_load_b128(rk, int(kvoff[u]), 0, 0);
#pragma unroll
    for (int u = 0; u < kAw8Req; u++) stg[kAw8Req + u] = __builtin_amdgcn_raw_buffer_load_b128(rv, int(vvoff[u]), 0, 0);
#else
    (void)rk, (void)rv;
#endif
  };
  // decode the staged codes and store them where the fp16 kernel's DMA writes the values
  auto commit = [&](int buf) {
    unsigned char* st = smemw8 + buf * kAwStage;
#pragma unroll
    for (int u = 0; u < kAw8Req; u++) {
      *reinterpret_cast<w8half8_t*>(st + attn_wide8_k_lds(w, u, l, 0)) = wide8_decode(stg[u][0], stg[u][1]);
      *reinterpret_cast<w8half8_t*>(st + attn_wide8_k_lds(w, u, l, 1)) = wide8_decode(stg[u][2], stg[u][3]);
    }
#pragma unroll
    for (int u = 0; u < kAw8Req; u++) {
      unsigned char* vd = st + attn_wide8_v_lds(w, u, l);
      *reinterpret_cast<w8half8_t*>(vd) = wide8_decode(stg[kAw8Req + u][0], stg[kAw8Req + u][1]);
      *reinterpret_cast<w8half8_t*>(vd + 16) = wide8_decode(stg[kAw8Req + u][2], stg[kAw8Req + u][3]);
    }
  };
  // operand addresses inside a stage
  const int swz_n = n & 15;
  const int k_rd = n * KROW;                                                                          // + 32 T rows, slot (2 j + h) ^ swizzle
  const int v_rd = kAwKTile + (4 * h + ((l & 15) >> 2)) * 64 + ((l >> 4) & 1) * 32 + (l & 3) * 8;  // + column block dt * 4 KiB, + 16-key step ts * 1 KiB, + 8 keys * 64

  const int nb = (kv_end + kA2KB - 1) / kA2KB;
  if (nb > 0) {
    idv = fetch_id(0);
    issue(0);
    commit(0);
  }
  __syncthreads();
  for (int b = 0; b < nb; b++) {
    const int pos0 = b * kA2KB;
    const bool more = b + 1 < nb;
    const unsigned char* sb = smemw8 + (b & 1) * kAwStage;
    if (wave_live && pos0 < vis_last) {
      // S^T = K(b) . Q^T: operands travel LDS -> registers one group of four MFMAs ahead of their use (two register sets, fenced)
      w8floatx16 sv[2];
#pragma unroll
      for (int T = 0; T < 2; T++)
#pragma unroll
        for (int i = 0; i < 16; i++) sv[T][i] = 0.f;
      {
        constexpr int CPT = NJ / 4, NCK = 2 * CPT;
        w8half8_t kf[2][4];
        auto ldk = [&](int c, w8half8_t(&dst)[4]) {
          const int T = c / CPT, j0 = (c % CPT) * 4;
#pragma unroll
          for (int u = 0; u < 4; u++) dst[u] = *reinterpret_cast<const w8half8_t*>(sb + k_rd + 32 * T * KROW + (((2 * (j0 + u) + h) ^ swz_n) << 4));
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
      if (more) issue(b + 1);
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
      w8half8_t pf[4];  // (T, s) -> 2 T + s
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
        w8half8_t vf[2][4];
        auto ldv = [&](int dt, w8half8_t(&dst)[4]) {
#pragma unroll
          for (int ts = 0; ts < 4; ts++) {
            const unsigned char* va = sb + v_rd + dt * 4096 + ts * 1024;
            const w8short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((w8short4_t __attribute__((address_space(3)))*)(va));
            const w8short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((w8short4_t __attribute__((address_space(3)))*)(va + 8 * 64));
            dst[ts] = __builtin_bit_cast(w8half8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
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
      issue(b + 1);
    }
    // tile b + 1 into the other stage, which every wave left at the last barrier; then every wave is done with tile b's stage
    if (more) commit((b + 1) & 1);
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
        const w8floatx4 y = w8floatx4{o[dt][4 * bq] * inv, o[dt][4 * bq + 1] * inv, o[dt][4 * bq + 2] * inv, o[dt][4 * bq + 3] * inv};
        if (aligned_dst) {
          *reinterpret_cast<w8floatx4*>(dr + d) = y;
          if (p.dst16) *reinterpret_cast<w8half4_t*>(p.dst16 + (dr - p.dst) + d) = w8half4_t{(_Float16)y[0], (_Float16)y[1], (_Float16)y[2], (_Float16)y[3]};
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

hipError_t launch_attn_prefill_paged_wide_f8(const AttnPrefillWidePlan& pl, hipStream_t st) {
  if (!pl.ok || !pl.f8) return hipErrorInvalidValue;
  if (pl.pad) return launch_lds<attn_wide_paged8_kernel<true>>(int(pl.lds), pl.grid, pl.block, pl.lds, st, pl.pp, pl.nqb, pl.aligned, pl.xcd_map);
  return launch_lds<attn_wide_paged8_kernel<false>>(int(pl.lds), pl.grid, pl.block, pl.lds, st, pl.pp, pl.nqb, pl.aligned, pl.xcd_map);
}

}  // namespace ns
