// ns_gemm2.hip — prefill / large-M GEMM, second generation:  C[M][N] = A[M][K] * dequant(W)      (MFMA-bound)
// (today: single matrices below "g3_min_m" rows or with NS_GEMM3=0 — ns_gemm_plan.cpp; the product is gemm3_kernel, ns_gemm3.hip — plus what both
// generations share: the split-K reduction and the fp32 -> fp16 pass over the activations)
//
// Design for MI355X (one workgroup = 256 threads = 4 waves, 256 x 128 output tile, 64-deep K chunks):
//   * each wave owns a 128 x 64 sub-tile = 8 x 4 v_mfma_f32_16x16x32_f16 accumulators (128 AGPR/VGPRs): per 32-deep
//     k-slice it reads 8 A and 4 B fragments from LDS for 32 MFMAs — at 64 x 64 per wave the four SIMDs of a CU ask
//     LDS for exactly its 128 B/clk, i.e. LDS would cap the kernel at the MFMA peak with no slack
//   * weights are dequantised ONCE per workgroup and chunk into LDS, already in MFMA B-fragment order and already
//     multiplied by their group scale (fp16: (code - zp) is an exact small integer, the product is rounded to 11 bits,
//     2^-12 relative, far inside the 1e-3 budget), so the inner loop is a pure MFMA accumulate chain — the first
//     generation applied the group scale to every MFMA result with 4 VALU FMAs, as much VALU time as MFMA time
//   * activations are fp16 in memory (caller's shadow, or one conversion pass into a per-stream scratch buffer that
//     is zero padded to the chunk size): 16-byte global loads, no conversion in the loop
//   * two LDS stages; the global loads of chunk c+1 are in flight while chunk c is multiplied; one barrier per chunk
//   * workgroup id -> (row block, column block) keeps the column blocks that share an XCD's L2 together
// Reference semantics: w = (code - zp) * scale, fp32 accumulate (bestla/bestla/kernel_ref.h:1027-1127 dequant,
// bestla_wrapper.h LauncherBase GEMM loop); A rounded to fp16 (north_star: fp16 activations).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ns_gemm.h"
#include "ns_launch.h"

namespace ns {

template <int KIND, int SPS, int SK, bool ASYM>
__global__ __launch_bounds__(256, NS_G2_OCC) void gemm2_kernel(const Gemm2Params p) {
  constexpr int NJ = (KIND == WK_INT8) ? 2 : 4;   // 32-deep slices per k-step record
  constexpr int CPS = NJ / 2;                      // 64-deep chunks per k-step
  constexpr int SBYTES = SPS * (SK == SK_F32 ? 4 : 2);
  using Corr = CorrRaw<SPS, SK, ASYM>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: keeps buffer soffsets in SGPRs
  const int l = tid & 63, nn = l & 15, g = l >> 4;
  const int wm = w >> 1, wn = w & 1;
  // workgroup -> (bm, bn): consecutive ids go to consecutive XCDs, so give each XCD its own run of column blocks and
  // let it sweep the row blocks: an XCD's L2 then holds its few column blocks' weights while A streams through once
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
  const int bn = xcd * p.cpx + local % p.cpx, bm = local / p.cpx;
  if (bn >= p.nbn) return;
  const int tile0 = bn * kG2Tiles, row0 = bm * kG2BM;

  const Rsrc rq = make_rsrc(p.codes, p.codes_bytes);
  const Rsrc rs = make_rsrc(p.scales, p.scales_bytes);
  const Rsrc rz = make_rsrc(p.zps, p.zps_bytes);
  const Rsrc ra = make_rsrc(p.a16, uint32_t(p.m) * uint32_t(p.lda16) * 2u);  // rows >= m read as zeros
  const I4Consts i4c = {0x000f000fu, 0x00f000f0u, 0x64006400u};

  floatx4 acc[kG2MI][4];
#pragma unroll
  for (int mi = 0; mi < kG2MI; mi++)
#pragma unroll
    for (int ni = 0; ni < 4; ni++) acc[mi][ni] = floatx4{0.f, 0.f, 0.f, 0.f};

  // ---- staging registers of the NEXT chunk ----
  uint4v areg[kG2MI];
  uint32_t breg[2][4];  // 16 weight codes per staging lane (INT8: 16 B; 4-bit: 8 B)
  Corr creg[2];

  auto load_chunk = [&](int c) {
    const int s = c / CPS, h = c % CPS;  // k-step record and its 64-deep half
#pragma unroll
    for (int it = 0; it < kG2MI; it++) {
      const int u = tid + 256 * it, r = u >> 3, ch = u & 7;
      const uint32_t off = (uint32_t(row0 + r) * uint32_t(p.lda16) + uint32_t(c * kG2KC + ch * 8)) * 2u;
      areg[it] = __builtin_bit_cast(uint4v, __builtin_amdgcn_raw_buffer_load_b128(ra, off, 0, 0));
    }
    const uint32_t srow = uint32_t(s * p.srow_mul) >> p.srow_shift;
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int tile = tile0 + w + 4 * r;
      const bool live = tile < p.ntiles;
      const uint32_t soff = (uint32_t(tile) * p.ksteps + s) * p.qstride;
      if constexpr (KIND == WK_INT8) {
        const uint4v v = live ? __builtin_bit_cast(uint4v, __builtin_amdgcn_raw_buffer_load_b128(rq, l * 16, soff, 0))
                              : uint4v{0, 0, 0, 0};
        breg[r][0] = v.x, breg[r][1] = v.y, breg[r][2] = v.z, breg[r][3] = v.w;
      } else {
        typedef uint32_t uint2v __attribute__((ext_vector_type(2)));
        const uint2v v = live ? __builtin_bit_cast(uint2v, __builtin_amdgcn_raw_buffer_load_b64(rq, l * 16 + 8 * h, soff, 0))
                              : uint2v{0x88888888u, 0x88888888u};
        breg[r][0] = v.x, breg[r][1] = v.y;
      }
      const uint32_t crow = uint32_t(live ? tile : 0) * p.srows + srow;
      corr_issue<SPS, SK, ASYM>(rs, rz, nn * SBYTES, nn * SPS, crow * p.sstride, crow * p.zstride, creg[r]);
    }
  };

  // registers -> LDS stage: A as is; B dequantised, scaled, in MFMA B-fragment order [tile][slice][g][nn] x 16 B
  auto store_chunk = [&](int c, unsigned char* stage) {
    const int h = c % CPS;
    _Float16* a_lds = reinterpret_cast<_Float16*>(stage);
    uint4v* b_lds = reinterpret_cast<uint4v*>(stage + kG2BM * kG2AStr * 2);
#pragma unroll
    for (int it = 0; it < kG2MI; it++) {
      const int u = tid + 256 * it, r = u >> 3, ch = u & 7;
      *reinterpret_cast<uint4v*>(a_lds + r * kG2AStr + ch * 8) = areg[it];
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int tl = w + 4 * r;
      float sc[4], zp[4];
      corr_decode<SPS, SK, ASYM, NJ>(creg[r], sc, zp);
#pragma unroll
      for (int jj = 0; jj < 2; jj++) {
        const int j = (KIND == WK_INT8) ? jj : 2 * h + jj;  // slice of the k-step record this chunk slice is
        // corr_decode fills sc[j] / zp[j] for j < 4 with compile-time indices only: select without dynamic indexing
        float s_j, z_j;
        if constexpr (KIND == WK_INT8) {
          s_j = sc[jj], z_j = zp[jj];
        } else {
          // bit select on registers: a ternary on the runtime `h` becomes a dynamically indexed scratch array
          const uint32_t hm = 0u - uint32_t(h);
          s_j = __builtin_bit_cast(float, (__builtin_bit_cast(uint32_t, sc[jj]) & ~hm) |
                                              (__builtin_bit_cast(uint32_t, sc[2 + jj]) & hm));
          z_j = __builtin_bit_cast(float, (__builtin_bit_cast(uint32_t, zp[jj]) & ~hm) |
                                              (__builtin_bit_cast(uint32_t, zp[2 + jj]) & hm));
        }
        (void)j;
        half8_t b;
        if constexpr (KIND == WK_INT4) {
          const _Float16 zl = (_Float16)(-1032.f - z_j), zh = (_Float16)(-72.f - z_j);
          b = cvt_i4x8(breg[r][jj], i4c, half2_t{zl, zl}, half2_t{zh, zh});
        } else if constexpr (KIND == WK_INT8) {
          const _Float16 zo = (_Float16)(-1152.f - z_j);
          b = cvt_i8x8(breg[r][2 * jj], breg[r][2 * jj + 1], half2_t{zo, zo});
        } else {
          b = cvt_f4x8(breg[r][jj], p.lut);
        }
        const _Float16 sh = (_Float16)(s_j * p.spre);
        b = b * half8_t{sh, sh, sh, sh, sh, sh, sh, sh};
        b_lds[((tl * 2 + jj) * 4 + g) * 16 + nn] = __builtin_bit_cast(uint4v, b);
      }
    }
  };

  auto compute = [&](const unsigned char* stage) {
    const _Float16* a_lds = reinterpret_cast<const _Float16*>(stage);
    const uint4v* b_lds = reinterpret_cast<const uint4v*>(stage + kG2BM * kG2AStr * 2);
    // all fragments of the chunk are requested up front (one wave per SIMD: nobody else hides the LDS latency);
    // the MFMAs of slice 0 then run while slice 1's fragments arrive
    half8_t bf[2][4], af[2][kG2MI];
#pragma unroll
    for (int jj = 0; jj < 2; jj++) {
#pragma unroll
      for (int ni = 0; ni < 4; ni++)
        bf[jj][ni] = __builtin_bit_cast(half8_t, b_lds[(((wn * 4 + ni) * 2 + jj) * 4 + g) * 16 + nn]);
#pragma unroll
      for (int mi = 0; mi < kG2MI; mi++)
        af[jj][mi] =
            *reinterpret_cast<const half8_t*>(a_lds + (wm * 16 * kG2MI + mi * 16 + nn) * kG2AStr + 32 * jj + 8 * g);
    }
    __builtin_amdgcn_sched_barrier(0);  // hipcc otherwise sinks each fragment load to just before its first MFMA
#pragma unroll
    for (int jj = 0; jj < 2; jj++)
#pragma unroll
      for (int mi = 0; mi < kG2MI; mi++)
#pragma unroll
        for (int ni = 0; ni < 4; ni++)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[jj][mi], bf[jj][ni], acc[mi][ni], 0, 0, 0);
  };

  unsigned char* stage0 = smem;
  const int cbeg = p.ksplit > 1 ? int(blockIdx.y) * p.cps : 0;
  const int cend = p.ksplit > 1 ? min(p.nchunks, cbeg + p.cps) : p.nchunks;
  if constexpr (kG2Stages == 2) {
    unsigned char* stage1 = smem + kG2StageBytes;
    load_chunk(cbeg);
    store_chunk(cbeg, stage0);
    __syncthreads();
    for (int c = cbeg; c < cend; c++) {
      unsigned char* cur = ((c - cbeg) & 1) ? stage1 : stage0;
      unsigned char* nxt = ((c - cbeg) & 1) ? stage0 : stage1;
      const bool more = c + 1 < cend;
      if (more) load_chunk(c + 1);
      compute(cur);
      if (more) store_chunk(c + 1, nxt);
      __syncthreads();
    }
  } else {
    load_chunk(cbeg);
    for (int c = cbeg; c < cend; c++) {
      store_chunk(c, stage0);
      __syncthreads();
      if (c + 1 < cend) load_chunk(c + 1);
      compute(stage0);
      __syncthreads();
    }
  }

  // ---- epilogue ----
#pragma unroll
  for (int mi = 0; mi < kG2MI; mi++)
#pragma unroll
    for (int ni = 0; ni < 4; ni++) {
      const int col = (tile0 + wn * 4 + ni) * 16 + nn;
      if (col >= p.n) continue;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = row0 + wm * 16 * kG2MI + mi * 16 + 4 * g + r;
        if (row >= p.m) continue;
        float v = acc[mi][ni][r] * p.spost;
        if (p.ksplit > 1) {  // raw partial; epilogue happens in gemm2_reduce_kernel
          p.part[(size_t(blockIdx.y) * p.m + row) * p.n + col] = v;
          continue;
        }
        const float dv = p.d ? p.d[size_t(row) * p.ldd + col] : 0.f;
        v = epi_apply(v, dv, p.epilogue);
        p.c[size_t(row) * p.ldc + col] = v;
        if (p.c16) p.c16[size_t(row) * p.ldc + col] = (_Float16)v;
      }
    }
}

// split-K tail: C = epilogue(sum over the K splits, in split order -> deterministic)
__global__ void gemm2_reduce_kernel(const Gemm2Params p) {
  const size_t idx = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= size_t(p.m) * p.n) return;
  const int row = int(idx / p.n), col = int(idx % p.n);
  float v = 0.f;
  for (int z = 0; z < p.ksplit; z++) v += p.part[(size_t(z) * p.m + row) * p.n + col];
  const float dv = p.d ? p.d[size_t(row) * p.ldd + col] : 0.f;
  v = epi_apply(v, dv, p.epilogue);
  p.c[size_t(row) * p.ldc + col] = v;
  if (p.c16) p.c16[size_t(row) * p.ldc + col] = (_Float16)v;
}

// fp32 [m][lda] -> fp16 [m][ld16], columns k..ld16-1 zero.  One thread per 8 outputs: two 16-byte loads, one 16-byte store.
__global__ void cvt_a16_kernel(const float* __restrict__ a, _Float16* __restrict__ out, int m, int k, int lda, int ld16) {
  const size_t idx = (size_t(blockIdx.x) * blockDim.x + threadIdx.x) * 8;
  const size_t total = size_t(m) * ld16;
  if (idx >= total) return;
  const int r = int(idx / ld16), c0 = int(idx % ld16);
  const float* src = a + size_t(r) * lda + c0;
  float f[8];
  if (c0 + 8 <= k && (lda & 3) == 0 && (reinterpret_cast<uintptr_t>(a) & 15) == 0) {
    const float4 v0 = *reinterpret_cast<const float4*>(src), v1 = *reinterpret_cast<const float4*>(src + 4);
    f[0] = v0.x, f[1] = v0.y, f[2] = v0.z, f[3] = v0.w, f[4] = v1.x, f[5] = v1.y, f[6] = v1.z, f[7] = v1.w;
  } else {
#pragma unroll
    for (int e = 0; e < 8; e++) f[e] = c0 + e < k ? src[e] : 0.f;
  }
  half2_t h[4];
#pragma unroll
  for (int e = 0; e < 4; e++) h[e] = half2_t{(_Float16)f[2 * e], (_Float16)f[2 * e + 1]};
  *reinterpret_cast<uint4v*>(out + idx) = uint4v{as_u32(h[0]), as_u32(h[1]), as_u32(h[2]), as_u32(h[3])};
}

hipError_t launch_cvt_a16(const float* a, void* out16, int m, int k, int lda, int ld16, hipStream_t st) {
  const size_t units = size_t(m) * ld16 / 8;
  hipLaunchKernelGGL(cvt_a16_kernel, dim3(unsigned((units + 255) / 256)), dim3(256), 0, st, a, static_cast<_Float16*>(out16), m,
                     k, lda, ld16);
  return hipGetLastError();
}

// the reduction pass of a launch that split K (e: the result of the main launch)
hipError_t launch_gemm_reduce(hipError_t e, const Gemm2Params& p, hipStream_t st) {
  if (e == hipSuccess && p.ksplit > 1) {
    const size_t total = size_t(p.m) * p.n;
    hipLaunchKernelGGL(gemm2_reduce_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, st, p);
    e = hipGetLastError();
  }
  return e;
}

// gemm2_kernel for the plan's format (with_format, ns_launch.h)
hipError_t launch_gemm2_plan(const GemmPlan& pl, hipStream_t st) {
  return with_format(pl.kind, pl.sps, pl.scale_dt, pl.asym, [&](auto kind_c, auto sps_c, auto sk_c, auto asym_c) {
    if constexpr (kind_c == WK_F8)
      return hipErrorNotSupported;  // (never planned: gemm2_kernel has no fp8 form)
    else
      return launch_gemm_reduce(launch_lds<gemm2_kernel<kind_c, sps_c, sk_c, asym_c>>(int(kG2Stages * kG2StageBytes), pl.grid, dim3(256), pl.lds, st, pl.p), pl.p, st);
  });
}

}  // namespace ns
