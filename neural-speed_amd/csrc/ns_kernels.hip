// ns_kernels.hip — hand-written gfx950 (MI355X / CDNA4) kernels of libns_hip.so.
//
//   repack_*        reference blob image  -> MI355X streaming layout            (load time, byte shuffling, HBM-bound)
//   smallm_kernel   C[M<=64][N] = A * dequant(W): weight-streaming MFMA kernel   (decode hot path, HBM-bound)
//   unpack_kernel   device layout -> fp32 [K][N]                                (bestla_unpackweight_fp32)
//   quant_* / pack_* fp32 -> codes/scales/zp -> reference blob image, bit-exact  (offline quantizer on the GPU)
//
// Reference semantics implemented (paths under /root/reference):
//   dequant   w = (code - zp) * scale            bestla/bestla/kernel_ref.h:1027-1127 (decompress_kblock_s4_fp)
//             w = LUT[code] * scale              kernel_ref.h:1456-1478 (decompress_kblock_f4_fp), LUTs bestla_utils.h:749-789
//   gemv      acc += a * w                       kernel_ref.h:2489-2531 (gemv_4bit_fp32_fp32)  [fp16 a, fp32 acc here]
//   quantize  per (k-block, column)              kernel_ref.h:1608-1719, :1801-1822
//   pack      interleave + bit planes + reduce   kernel_ref.h:39-57, :155-365, :2132-2142; bestla_prologue_b.h:378-617
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "ns_common.h"
#include "ns_dev.h"
#include "ns_launch.h"

namespace ns {

// element (k, n) of the reference's interleaved image: [N/NTILE][KPad/PACK][NTILE][PACK]
// (padding_interleave kernel_ref.h:39-57 as driven by reorderWeight bestla_prologue_b.h:490-510)
__device__ __forceinline__ size_t ref_tiled_index(int k, int n, int ntile, int packrow, int kpad) {
  return size_t(n / ntile) * ntile * kpad + size_t(k / packrow) * ntile * packrow + size_t(n % ntile) * packrow +
         (k % packrow);
}
// unsigned stored code of element e of a reference bit-plane image (compress_*, kernel_ref.h:155-365;
// plane offsets bestla_prologue_b.h:512-547).  4/8-bit and f4 have a single plane.
__device__ __forceinline__ int ref_stored_code(const uint8_t* img, size_t e, size_t elts, int bits) {
  if (bits == 8) return img[e];
  if (bits == 4) return (img[e >> 1] >> ((e & 1) * 4)) & 0xf;
  const uint8_t* p = img;
  int v = 0, sh = 0;
  if (bits & 4) {
    v |= (p[e >> 1] >> ((e & 1) * 4)) & 0xf;
    p += elts / 2;
    sh = 4;
  }
  if (bits & 2) {
    v |= ((p[e >> 2] >> ((e & 3) * 2)) & 0x3) << sh;
    p += elts / 4;
    sh += 2;
  }
  if (bits & 1) v |= ((p[e >> 3] >> (e & 7)) & 0x1) << sh;
  return v;
}

// ============================================================================================================
// repack: reference blob sections -> device streaming layout (see ns_common.h ns_weight)
// ============================================================================================================
__global__ void repack_codes_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ out, uint32_t qstride, int n,
                                    int k, int ntiles, int ksteps, int kind, int ref_bits, int ref_ntile,
                                    int ref_packrow, int ref_kpad, int ref_npad, uint32_t* __restrict__ bad_e5m2) {
  // one thread per output dword
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t total = size_t(ntiles) * ksteps * 64 * 4;
  if (gid >= total) return;
  const int d = int(gid & 3);
  const int lane = int((gid >> 2) & 63);
  const size_t ts = gid >> 8;
  const int s = int(ts % ksteps);
  const int t = int(ts / ksteps);
  const int nn = lane & 15, c = lane >> 4;
  const int col = t * 16 + nn;
  const size_t elts = size_t(ref_npad) * ref_kpad;
  uint32_t word = 0;
  // integer types narrower than the device container (1-3 bit in nibbles, 5-7 bit in bytes) are widened here: the
  // reference stores code + 2^(b-1) in bit planes (decompress_s{1..7}_s8, kernel_ref.h:367-526)
  const int full = 1 << (ref_bits - 1);
  if (kind == WK_INT8 || kind == WK_F8) {
    // dword d of the lane: j = d >> 1, bytes i = (d & 1) * 4 .. +3 ; k = s*64 + 32*j + 8*c + i
    const int j = d >> 1;
    for (int b = 0; b < 4; b++) {
      const int kk = s * 64 + 32 * j + 8 * c + (d & 1) * 4 + b;
      int q = 0;
      if (kk < k && col < n) {
        const size_t e = ref_tiled_index(kk, col, ref_ntile, ref_packrow, ref_kpad);
        q = ref_bits == 8 ? int(img[e]) : ref_stored_code(img, e, elts, ref_bits) - full;
        // E5M2 codes with exponent field 31 (>= 65536 before scaling) do not fit fp16; the reference quantizer never
        // emits them (max_norm = 57344, kernel_ref.h:1743-1744) — flag them so that the load fails loudly
        if (bad_e5m2 && (q & 0x7c) == 0x7c) atomicOr(bad_e5m2, 1u);
      }
      word |= uint32_t(q & 0xff) << (8 * b);
    }
  } else {
    // dword j = d: k = s*128 + 32*j + 8*c + i
    const int zero_code = (kind == WK_INT4) ? 8 : 0;  // int4 stores code+8 (compress_s8_s4); f4 code 0 decodes to 0.0
    const int rebias = (kind == WK_INT4) ? 8 - full : 0;  // 0 for 4-bit
    for (int i = 0; i < 8; i++) {
      const int kk = s * 128 + 32 * d + 8 * c + i;
      int u = zero_code;
      if (kk < k && col < n)
        u = ref_stored_code(img, ref_tiled_index(kk, col, ref_ntile, ref_packrow, ref_kpad), elts, ref_bits) + rebias;
      word |= uint32_t(u & 0xf) << nib_shift(i);
    }
  }
  *reinterpret_cast<uint32_t*>(out + ts * qstride + size_t(lane) * 16 + d * 4) = word;
}

// Native bit-plane records (ns_common.h ns_weight::native; decode kernel: gemv_kernel<..., PL = true>).  One record = the planes of
// one k-step of a 16-column tile, back to back, every plane indexed by lane l = (column nn = l & 15, k-slot c = l >> 4) and laid
// out so that the kernel rebuilds its nibble / byte container words with shifts and masks only.  Codes are the reference's STORED
// codes (q + 2^(bits-1)); columns and k past the matrix hold the code of zero.
//   nibble order (S1..S3; 128 k per k-step; the lane's 32 codes = words j = 0..3 x nibbles i = 0..7, k = 128 s + 32 j + 8 c + i):
//     2-bit plane, 8 B per lane at 8 l: word j >> 1 holds bits 0..1 of code (j, i) at bit nib_shift(i) + 2 (j & 1)
//     1-bit plane, 4 B per lane (at 512 + 4 l behind a 2-bit plane, else at 4 l): top bit of code (j, i) at bit nib_shift(i) + j
//   byte order (S5..S7; 64 k per k-step; the lane's 16 codes = words d = 0..3 x bytes b = 0..3, k = 64 s + 32 (d >> 1) + 8 c + 4 (d & 1) + b):
//     4-bit plane, 8 B per lane at 8 l: word d >> 1 holds bits 0..3 of code (d, b) at bit 8 b + 4 (d & 1)
//     2-bit plane (S6), 4 B per lane at 512 + 4 l: bits 4..5 of code (d, b) at bit 8 b + 2 d
//     1-bit plane (S5), 4 B per lane at 512 + 4 l: bit 4 of code (d, b) at bit 8 b + d
//   (S7 has no native form: 4 + 2 + 1 bit planes in whole words per lane are as long as the byte record)
__global__ void repack_planes_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ out, uint32_t qstride, int n, int k,
                                     int ntiles, int ksteps, int bits, int ref_ntile, int ref_packrow, int ref_kpad, int ref_npad) {
  // one thread per (record, lane)
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t total = size_t(ntiles) * ksteps * 64;
  if (gid >= total) return;
  const int lane = int(gid & 63);
  const size_t ts = gid >> 6;
  const int s = int(ts % ksteps), t = int(ts / ksteps);
  const int nn = lane & 15, c = lane >> 4;
  const int col = t * 16 + nn;
  const size_t elts = size_t(ref_npad) * ref_kpad;
  const int full = 1 << (bits - 1);
  uint8_t* rec = out + ts * qstride;
  auto code = [&](int kk) {
    return (kk < k && col < n) ? ref_stored_code(img, ref_tiled_index(kk, col, ref_ntile, ref_packrow, ref_kpad), elts, bits) : full;
  };
  if (bits <= 3) {
    uint32_t a[2] = {0, 0}, cw = 0;
    for (int j = 0; j < 4; j++)
      for (int i = 0; i < 8; i++) {
        const uint32_t u = uint32_t(code(s * 128 + 32 * j + 8 * c + i));
        if (bits >= 2) a[j >> 1] |= (u & 3u) << (nib_shift(i) + 2 * (j & 1));
        if (bits != 2) cw |= ((u >> (bits - 1)) & 1u) << (nib_shift(i) + j);
      }
    if (bits >= 2) {
      reinterpret_cast<uint32_t*>(rec + 8 * lane)[0] = a[0];
      reinterpret_cast<uint32_t*>(rec + 8 * lane)[1] = a[1];
    }
    if (bits != 2) *reinterpret_cast<uint32_t*>(rec + (bits == 3 ? 512 : 0) + 4 * lane) = cw;
  } else {
    uint32_t nw[2] = {0, 0}, pw = 0, hw = 0;
    for (int d = 0; d < 4; d++)
      for (int b = 0; b < 4; b++) {
        const uint32_t u = uint32_t(code(s * 64 + 32 * (d >> 1) + 8 * c + 4 * (d & 1) + b));
        nw[d >> 1] |= (u & 15u) << (8 * b + 4 * (d & 1));
        if (bits == 6) pw |= ((u >> 4) & 3u) << (8 * b + 2 * d);
        if (bits == 5) hw |= ((u >> 4) & 1u) << (8 * b + d);
      }
    reinterpret_cast<uint32_t*>(rec + 8 * lane)[0] = nw[0];
    reinterpret_cast<uint32_t*>(rec + 8 * lane)[1] = nw[1];
    *reinterpret_cast<uint32_t*>(rec + 512 + 4 * lane) = bits == 6 ? pw : hw;
  }
}

// scales / zero points: reference [nblk][cstep] -> [ntiles][G][16][SPS]
template <typename T>
__global__ void repack_corr_kernel(const T* __restrict__ src, uint8_t* __restrict__ dst, uint32_t rstride, int n,
                                   int ntiles, int srows, int sps, int cstep, int ref_nblk) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t total = size_t(ntiles) * srows * 16 * sps;
  if (gid >= total) return;
  const int sp = int(gid % sps);
  const int nn = int((gid / sps) % 16);
  const int row = int((gid / (size_t(sps) * 16)) % srows);
  const int t = int(gid / (size_t(sps) * 16 * srows));
  const int kb = row * sps + sp;
  const int col = t * 16 + nn;
  T v = T(0);
  if (kb < ref_nblk && col < n) v = src[size_t(kb) * cstep + col];
  *reinterpret_cast<T*>(dst + (size_t(t) * srows + row) * rstride + (size_t(nn) * sps + sp) * sizeof(T)) = v;
}

// E8M0 shared exponents -> fp32 scales 2^e (e = -127 is the fp32 subnormal 2^-127), same destination layout
__device__ __forceinline__ uint32_t e8m0_bits(int e) { return e > -127 ? uint32_t(e + 127) << 23 : 0x00400000u; }
__global__ void repack_e8m0_kernel(const int8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t rstride, int n,
                                   int ntiles, int srows, int sps, int cstep, int ref_nblk) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t total = size_t(ntiles) * srows * 16 * sps;
  if (gid >= total) return;
  const int sp = int(gid % sps);
  const int nn = int((gid / sps) % 16);
  const int row = int((gid / (size_t(sps) * 16)) % srows);
  const int t = int(gid / (size_t(sps) * 16 * srows));
  const int kb = row * sps + sp;
  const int col = t * 16 + nn;
  uint32_t v = 0;
  if (kb < ref_nblk && col < n) v = e8m0_bits(src[size_t(kb) * cstep + col]);
  *reinterpret_cast<uint32_t*>(dst + (size_t(t) * srows + row) * rstride + (size_t(nn) * sps + sp) * 4) = v;
}

hipError_t launch_repack(const RepackArgs& a, ns_weight* w, hipStream_t st) {
  const size_t dwords = size_t(w->ntiles) * w->ksteps * 64 * 4;
  const int ref_bits = dt_bits(w->qtype);
  if (w->pl_bits)  // a native clone: the format's own planes instead of the widened record
    hipLaunchKernelGGL(repack_planes_kernel, dim3((dwords / 4 + 255) / 256), dim3(256), 0, st, a.q, (uint8_t*)w->codes, w->qstride, w->n,
                       w->k, w->ntiles, w->ksteps, int(w->pl_bits), a.ref_ntile, a.ref_packrow, a.ref_kpad, a.ref_npad);
  else
    hipLaunchKernelGGL(repack_codes_kernel, dim3((dwords + 255) / 256), dim3(256), 0, st, a.q, (uint8_t*)w->codes,
                       w->qstride, w->n, w->k, w->ntiles, w->ksteps, w->kind, ref_bits, a.ref_ntile, a.ref_packrow,
                       a.ref_kpad, a.ref_npad, w->qtype == DT_F8_E5M2 ? a.flags : nullptr);
  const size_t nsc = size_t(w->ntiles) * w->srows * 16 * w->sps;
  if (a.src_scale_dt == DT_F8_E8M0)
    hipLaunchKernelGGL(repack_e8m0_kernel, dim3((nsc + 255) / 256), dim3(256), 0, st, (const int8_t*)a.scales,
                       (uint8_t*)w->scales, w->sstride, w->n, w->ntiles, w->srows, w->sps, a.cstep, a.ref_nblk);
  else if (w->scale_dt == DT_F32)
    hipLaunchKernelGGL(repack_corr_kernel<uint32_t>, dim3((nsc + 255) / 256), dim3(256), 0, st,
                       (const uint32_t*)a.scales, (uint8_t*)w->scales, w->sstride, w->n, w->ntiles, w->srows, w->sps,
                       a.cstep, a.ref_nblk);
  else
    hipLaunchKernelGGL(repack_corr_kernel<uint16_t>, dim3((nsc + 255) / 256), dim3(256), 0, st,
                       (const uint16_t*)a.scales, (uint8_t*)w->scales, w->sstride, w->n, w->ntiles, w->srows, w->sps,
                       a.cstep, a.ref_nblk);
  if (w->asym)
    hipLaunchKernelGGL(repack_corr_kernel<int8_t>, dim3((nsc + 255) / 256), dim3(256), 0, st, a.zps, (uint8_t*)w->zps,
                       w->zstride, w->n, w->ntiles, w->srows, w->sps, a.cstep, a.ref_nblk);
  return hipGetLastError();
}

// largest finite |scale| of a reference scale section; positive fp32 bit patterns order like unsigned integers.  cstep > 0: rows of
// cstep entries of which the first n are columns of the weight — the padding behind them is skipped (its zero BYTES are zero scales
// in the float types but 2^0 as a shared exponent)
__global__ void scale_absmax_kernel(const uint8_t* __restrict__ s, size_t count, uint32_t scale_dt, uint32_t* out, int cstep, int n) {
  uint32_t best = 0;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += size_t(gridDim.x) * blockDim.x) {
    if (cstep > 0 && int(i % size_t(cstep)) >= n) continue;
    uint32_t bits;
    if (scale_dt == DT_F8_E8M0) {
      bits = e8m0_bits(reinterpret_cast<const int8_t*>(s)[i]);
    } else if (scale_dt == DT_F32) {
      bits = reinterpret_cast<const uint32_t*>(s)[i];
    } else if (scale_dt == DT_BF16) {
      bits = uint32_t(reinterpret_cast<const uint16_t*>(s)[i]) << 16;
    } else {
      bits = __builtin_bit_cast(uint32_t, float(reinterpret_cast<const _Float16*>(s)[i]));
    }
    bits &= 0x7fffffffu;
    if (bits < 0x7f800000u && bits > best) best = bits;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = uint32_t(__shfl_xor(int(best), o));
    best = other > best ? other : best;
  }
  if ((threadIdx.x & 63) == 0 && best) atomicMax(out, best);
}
hipError_t launch_scale_absmax(const void* scales, size_t count, uint32_t scale_dt, uint32_t* out_bits, hipStream_t st, int cstep, int n) {
  if (!count) return hipSuccess;
  const unsigned blocks = unsigned(std::min<size_t>((count + 255) / 256, 1024));
  hipLaunchKernelGGL(scale_absmax_kernel, dim3(blocks), dim3(256), 0, st, static_cast<const uint8_t*>(scales), count,
                     scale_dt, out_bits, cstep, n);
  return hipGetLastError();
}

// fp8 weights on the tiled GEMM (ns_gemm3.hip): does any non-zero finite |scale| lie below 2^(e - drop), smax = f * 2^e with f in [0.5, 1)?
// `info[0]` = the largest |scale| (scale_absmax_kernel, earlier on the same stream); bit 1 of info[1] is set when one does.
__global__ void scale_spread_kernel(const uint8_t* __restrict__ s, size_t count, uint32_t scale_dt, int drop, uint32_t* info, int cstep, int n) {
  const int e = int((info[0] >> 23) & 0xffu) - 126;
  const int biased = e - drop + 127;
  if (biased <= 0) return;  // the bound is below fp32's normal range
  const uint32_t thr = uint32_t(biased) << 23;
  bool low = false;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += size_t(gridDim.x) * blockDim.x) {
    if (cstep > 0 && int(i % size_t(cstep)) >= n) continue;
    uint32_t bits = scale_dt == DT_F8_E8M0 ? e8m0_bits(reinterpret_cast<const int8_t*>(s)[i]) : reinterpret_cast<const uint32_t*>(s)[i];
    bits &= 0x7fffffffu;
    low |= bits != 0 && bits < thr;
  }
  if (__any(low) && (threadIdx.x & 63) == 0) atomicOr(info + 1, 2u);
}
hipError_t launch_scale_spread(const void* scales, size_t count, uint32_t scale_dt, int drop, uint32_t* info, hipStream_t st, int cstep, int n) {
  if (!count) return hipSuccess;
  const unsigned blocks = unsigned(std::min<size_t>((count + 255) / 256, 1024));
  hipLaunchKernelGGL(scale_spread_kernel, dim3(blocks), dim3(256), 0, st, static_cast<const uint8_t*>(scales), count, scale_dt, drop, info, cstep, n);
  return hipGetLastError();
}

// ============================================================================================================
// smallm_kernel — weight-streaming MFMA kernel for M <= 16*MB rows (decode / batched decode)
//
// One workgroup = NW waves = one 16-column tile (or the same tile of two matrices in DUAL mode) over the whole K.
// Wave w streams k-steps w, w+NW, ...: one 16-byte load per lane per k-step = 1 KiB contiguous per wave-load,
// kPF k-steps (codes + scales) in flight per wave, refilled as they are consumed.
// Lane (nn = l&15, c = l>>4) is column nn of the tile and k-slot c of the MFMA: its 16 B are the B operand of
// NJ = 4 (4-bit) / 2 (8-bit) v_mfma_f32_16x16x32_f16, one per 32-deep k-slice j, so that every MFMA lives inside
// one quantisation group (blocksize % 32 == 0) and the group scale is applied to the fp32 MFMA result:
//     acc += scale[j][nn] * mfma(A_frag(j), codes(j) - zp, 0)
// exactly the reference's w = (code - zp) * scale with fp32 accumulation (kernel_ref.h:2489-2531), except that
// A is rounded to fp16 (north_star: fp16 activations).  A is staged once per workgroup in LDS as fp16.
// ============================================================================================================
constexpr int kMaxNW = 16;  // waves per workgroup: 4, 8 or 16 (runtime, blockDim.x / 64)
#ifndef NS_PF
#define NS_PF 4
#endif
constexpr int kPF = NS_PF;  // k-steps each wave keeps in flight (codes + scales [+ zero points])
#ifndef NS_PF_WIDE
#define NS_PF_WIDE 2
#endif
constexpr int kPFWide = NS_PF_WIDE;  // same for the 16-wave variant
#ifndef NS_A16F_WIDE
#define NS_A16F_WIDE 0
#endif
constexpr bool kA16FirstWide = NS_A16F_WIDE != 0;  // fetch the fp16 shadow ahead of the ring in the 16-wave variant too

struct SmallMParams {
  const float* a;
  const _Float16* a16;  // optional fp16 shadow of A
  _Float16* c16[3];     // optional fp16 shadow of C
  int lda, m, k;
  int ksteps;       // k-steps of the weight (kpad / KSTEP)
  int chunk_steps;  // k-steps staged in LDS at a time (multiple of NW)
  int nseg;
  int tile_begin[4];  // first global tile of each segment (+ total)
  const uint4* codes[3];
  const void* scales[3];
  const int8_t* zps[3];
  uint32_t codes_bytes[3], scales_bytes[3], zps_bytes[3];  // buffer-descriptor extents (each < 4 GiB)
  uint32_t qstride, sstride, zstride;                      // ns_weight strides (interleaved records or 3 arrays)
#ifdef NS_TRACE
  unsigned long long* trace;  // diagnostics build: [block][16 waves][8] wall-clock stamps (100 MHz)
#endif
  float* c[3];
  int n[3];
  int ldc;
  uint32_t scale_dt;
  int srows;
  int srow_mul, srow_shift;  // scale row of k-step s = (s * srow_mul) >> srow_shift  (branch-free s / ratio)
  int epilogue;
  const float* d;
  int ldd;
  float* c2;
  F4Lut lut;
  F8Consts f8;
};
// diagnostics only: build with -DNS_ABLATE=n (1 = no dequant/MFMA, 2 = no scale loads, 4 = no A staging)
#ifndef NS_ABLATE
#define NS_ABLATE 0
#endif
constexpr int kAblate = NS_ABLATE;

#ifdef NS_TRACE
#define NS_STAMP(i)                                                                                      \
  do {                                                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096)                                                     \
      p.trace[(size_t(blockIdx.x) * 16 + (threadIdx.x >> 6)) * 8 + (i)] = wall_clock64();                 \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
  } while (0)
#else
#define NS_STAMP(i)
#endif
template <int KIND, int SPS, int MB, bool DUAL, int SK, bool ASYM, bool WIDE>
#ifndef NS_WPE1
#define NS_WPE1 4
#endif
#ifndef NS_WPE2
#define NS_WPE2 4
#endif
// WIDE = launched with 16 waves (1024 threads): caps the kernel at 128 VGPRs; the common <= 8-wave instantiation may
// use more registers (no spills) at 2-3 waves per SIMD, which the kPF-deep load ring makes sufficient
__global__ __launch_bounds__(WIDE ? kMaxNW * 64 : 512) void smallm_kernel(const SmallMParams p) {
  constexpr int NJ = kind_is_8bit(KIND) ? 2 : 4;
  constexpr int KSTEP = NJ * 32;
  constexpr int NQ = DUAL ? 2 : 1;  // matrices streamed by one workgroup
  // ring depth: the 16-wave (WIDE) variant already has 16 x 2 KiB per workgroup in flight and is capped at 128 VGPRs;
  // a 2-deep ring measured faster there (down projection 9.2 -> 8.6 us) and does not spill
  constexpr int PF = (WIDE || MB == 4) ? kPFWide : kPF;  // MB == 4: the 4-deep ring spilled 556 B per lane
  static_assert(PF % NQ == 0, "ring slots alternate between the two matrices");
  constexpr int SBYTES = SPS * (SK == SK_F32 ? 4 : 2);
  using Corr = CorrRaw<SPS, SK, ASYM>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  _Float16* a_lds = reinterpret_cast<_Float16*>(smem);

  NS_STAMP(0);
  const int tid = threadIdx.x;
  const int NW = blockDim.x >> 6;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = tid & 63;
  const int nn = l & 15, g = l >> 4;

  // which segment / tile; descriptors of the matrices this workgroup streams are built ONCE from scalars
  int seg = 0;
  int tile = blockIdx.x;
  if (!DUAL) {
    if (p.nseg > 1 && tile >= p.tile_begin[1]) seg = 1;
    if (p.nseg > 2 && tile >= p.tile_begin[2]) seg = 2;
    tile -= p.tile_begin[seg];
  }
  Rsrc rq[NQ], rs[NQ], rz[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    const int sg = DUAL ? q : seg;
    rq[q] = make_rsrc(sg == 0 ? p.codes[0] : (sg == 1 ? p.codes[1] : p.codes[2]),
                      sg == 0 ? p.codes_bytes[0] : (sg == 1 ? p.codes_bytes[1] : p.codes_bytes[2]));
    rs[q] = make_rsrc(sg == 0 ? p.scales[0] : (sg == 1 ? p.scales[1] : p.scales[2]),
                      sg == 0 ? p.scales_bytes[0] : (sg == 1 ? p.scales_bytes[1] : p.scales_bytes[2]));
    rz[q] = make_rsrc(sg == 0 ? p.zps[0] : (sg == 1 ? p.zps[1] : p.zps[2]),
                      sg == 0 ? p.zps_bytes[0] : (sg == 1 ? p.zps_bytes[1] : p.zps_bytes[2]));
  }
  const uint32_t voff_q = l * 16, voff_s = nn * SBYTES, voff_z = nn * SPS;  // the only per-lane address parts
  const uint32_t tile_q = uint32_t(tile) * p.ksteps * p.qstride;            // + s * qstride
  const uint32_t tile_c = uint32_t(tile) * p.srows;                         // + srow, times sstride / zstride
  const I4Consts i4c = {0x000f000fu, 0x00f000f0u, 0x64006400u};

  const int rows = min(p.m, 16 * MB);
  const int chunk_k = p.chunk_steps * KSTEP;
  const int row_stride = chunk_k + 8;  // halves; +16 B keeps 16-B alignment and skews banks

  floatx4 acc[NQ][MB];
#pragma unroll
  for (int q = 0; q < NQ; q++)
#pragma unroll
    for (int mb = 0; mb < MB; mb++) acc[q][mb] = floatx4{0.f, 0.f, 0.f, 0.f};

  // A-fragment LDS offsets of this lane (rows >= m are clamped: their output rows are discarded)
  int aoff[MB];
#pragma unroll
  for (int mb = 0; mb < MB; mb++) aoff[mb] = min(mb * 16 + nn, rows - 1) * row_stride + 8 * g;

  // ring of kPF in-flight items; item t of a wave = (k-step ordinal t / NQ, matrix t % NQ); slot i always holds
  // matrix i % NQ, so every register index below is a compile-time constant
  uint4v qv[PF];
  Corr cr[PF];

  auto issue = [&](auto slot_c, int s) {
    constexpr int slot = decltype(slot_c)::value;
    constexpr int q = slot % NQ;
    const uint32_t srow = uint32_t(s * p.srow_mul) >> p.srow_shift;
    qv[slot] = __builtin_bit_cast(uint4v, __builtin_amdgcn_raw_buffer_load_b128(rq[q], voff_q, tile_q + uint32_t(s) * p.qstride, 2));
    if constexpr (kAblate & 2) {
#pragma unroll
      for (int i = 0; i < Corr::NW32; i++) cr[slot].s[i] = 0x3c003c00u;
      if constexpr (ASYM) cr[slot].z[0] = 0;
    } else {
      const uint32_t crow = tile_c + srow;
      corr_issue<SPS, SK, ASYM>(rs[q], rz[q], voff_s, voff_z, crow * p.sstride, crow * p.zstride, cr[slot]);
    }
  };

  auto compute = [&](auto slot_c, int s_local) {
    constexpr int slot = decltype(slot_c)::value;
    constexpr int q = slot % NQ;
    if constexpr (kAblate & 1) {  // diagnostics: keep the loads alive, skip all math
      acc[q][0][0] += __builtin_bit_cast(float, (qv[slot].x ^ qv[slot].y ^ qv[slot].z ^ qv[slot].w ^ cr[slot].s[0]) & 0x007fffffu);
      return;
    }
    const _Float16* abase = a_lds + s_local * KSTEP;
    float sc[4], zp[4];
    corr_decode<SPS, SK, ASYM, NJ>(cr[slot], sc, zp);
    const uint32_t xw[4] = {qv[slot].x, qv[slot].y, qv[slot].z, qv[slot].w};
    // dequantise all slices first, then issue the MFMAs back to back (independent accumulators), then scale:
    // no MFMA-result -> VALU stall in between
    half8_t b[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      if constexpr (KIND == WK_INT4) {
        const _Float16 zl = (_Float16)(-1032.f - zp[j]), zh = (_Float16)(-72.f - zp[j]);
        b[j] = cvt_i4x8(xw[j], i4c, half2_t{zl, zl}, half2_t{zh, zh});
      } else if constexpr (KIND == WK_INT8) {
        const _Float16 zo = (_Float16)(-1152.f - zp[j]);
        b[j] = cvt_i8x8(xw[2 * j], xw[2 * j + 1], half2_t{zo, zo});
      } else if constexpr (KIND == WK_F8) {
        b[j] = cvt_f8x8(xw[2 * j], xw[2 * j + 1], p.f8);
      } else {
        b[j] = cvt_f4x8(xw[j], p.lut);
      }
    }
#pragma unroll
    for (int mb = 0; mb < MB; mb++) {
      floatx4 dd[NJ];
#pragma unroll
      for (int j = 0; j < NJ; j++) {
        const half8_t afrag = *reinterpret_cast<const half8_t*>(abase + aoff[mb] + 32 * j);
        dd[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afrag, b[j], floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < NJ; j++) acc[q][mb] += dd[j] * sc[j];
    }
  };

  for (int c0 = 0; c0 < p.ksteps; c0 += p.chunk_steps) {
    const int cend = min(c0 + p.chunk_steps, p.ksteps);
    const int first = c0 + w;
    const int nst = first < cend ? (cend - first + NW - 1) / NW : 0;  // this wave's k-steps in the chunk
    const int nitems = nst * NQ;
    const int sl0 = first - c0;
    // step of item t: first + (t / NQ) * NW
    // ---- put the wave's first kPF items in flight BEFORE staging A: nothing below depends on them until
    //      compute(), so HBM latency overlaps the staging, the barrier and the other waves.
    //      The common case (nitems >= kPF) issues unconditionally so the compiler knows what is outstanding ----
    const bool full_pipe = nitems >= PF;
    const int quads = chunk_k >> 2;
    // fp16 shadow available and small enough to sit in two registers per thread: fetch it BEFORE the weight ring so
    // it retires first (vmcnt is in order) and the staging + barrier complete while the weights are in flight
    const int octs = chunk_k >> 3;  // 16-byte units per row
    constexpr int kA16It = 4;
    const bool a16_first = (!WIDE || kA16FirstWide) && p.a16 != nullptr && rows * octs <= kA16It * int(blockDim.x) && (p.lda & 7) == 0 &&
                           ((reinterpret_cast<uintptr_t>(p.a16) & 15) == 0);
    uint4v a16r[kA16It];
    if (a16_first) {
      const Rsrc ra = make_rsrc(p.a16, uint32_t(rows) * uint32_t(p.lda) * 2u);
#pragma unroll
      for (int it = 0; it < kA16It; it++) {
        const int idx = tid + it * int(blockDim.x);
        const int r = idx / octs, ko = idx - r * octs;
        // beyond K (tail k-step) the row's own tail or the next row would be read: mask by range below
        const uint32_t off = (uint32_t(r) * p.lda + uint32_t(c0 * KSTEP + ko * 8)) * 2u;
        a16r[it] = (idx < rows * octs) ? __builtin_bit_cast(uint4v, __builtin_amdgcn_raw_buffer_load_b128(ra, off, 0, 0))
                                       : uint4v{0, 0, 0, 0};
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (full_pipe) {
      NS_FOR_SLOTS({ issue(ic, first + (i / NQ) * NW); })
    } else {
      NS_FOR_SLOTS({ if (i < nitems) issue(ic, first + (i / NQ) * NW); })
    }
    __builtin_amdgcn_sched_barrier(0);
    NS_STAMP(1);
    // ---- stage A[:, chunk] as fp16 ----
    if (c0 > 0) __syncthreads();
    if constexpr (!(kAblate & 4)) {
      if (a16_first) {
#pragma unroll
        for (int it = 0; it < kA16It; it++) {
          const int idx = tid + it * int(blockDim.x);
          const int r = idx / octs, ko = idx - r * octs;
          uint4v v = a16r[it];
          const int gk = c0 * KSTEP + ko * 8;
          if (gk + 8 > p.k) {  // zero the part of the last unit that lies beyond K
            uint32_t* vw = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
            for (int e = 0; e < 8; e++)
              if (gk + e >= p.k) vw[e >> 1] &= (e & 1) ? 0x0000ffffu : 0xffff0000u;
          }
          if (idx < rows * octs) *reinterpret_cast<uint4v*>(a_lds + size_t(r) * row_stride + ko * 8) = v;
        }
      } else if (p.a16 != nullptr && (p.lda & 7) == 0 && ((reinterpret_cast<uintptr_t>(p.a16) & 15) == 0)) {
        const Rsrc ra = make_rsrc(p.a16, uint32_t(rows) * uint32_t(p.lda) * 2u);
        for (int idx = tid; idx < rows * octs; idx += blockDim.x) {
          const int r = idx / octs, ko = idx - r * octs;
          const int gk = c0 * KSTEP + ko * 8;
          uint4v v = __builtin_bit_cast(uint4v, __builtin_amdgcn_raw_buffer_load_b128(
                                                    ra, (uint32_t(r) * p.lda + uint32_t(gk)) * 2u, 0, 0));
          if (gk + 8 > p.k) {
            uint32_t* vw = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
            for (int e = 0; e < 8; e++)
              if (gk + e >= p.k) vw[e >> 1] &= (e & 1) ? 0x0000ffffu : 0xffff0000u;
          }
          *reinterpret_cast<uint4v*>(a_lds + size_t(r) * row_stride + ko * 8) = v;
        }
      } else {
        const int kbase = c0 * KSTEP;
        const bool vec_ok = ((p.lda & 3) == 0) && ((reinterpret_cast<uintptr_t>(p.a) & 15) == 0);
        for (int idx = tid; idx < rows * quads; idx += blockDim.x) {
          const int r = idx / quads;
          const int kq = (idx - r * quads) << 2;
          const int gk = kbase + kq;
          float4 v = {0.f, 0.f, 0.f, 0.f};
          const float* src = p.a + size_t(r) * p.lda + gk;
          if (vec_ok && gk + 3 < p.k) {
            v = *reinterpret_cast<const float4*>(src);
          } else {
            if (gk + 0 < p.k) v.x = src[0];
            if (gk + 1 < p.k) v.y = src[1];
            if (gk + 2 < p.k) v.z = src[2];
            if (gk + 3 < p.k) v.w = src[3];
          }
          half2_t h0 = {(_Float16)v.x, (_Float16)v.y}, h1 = {(_Float16)v.z, (_Float16)v.w};
          uint2 packed = {as_u32(h0), as_u32(h1)};
          *reinterpret_cast<uint2*>(a_lds + size_t(r) * row_stride + kq) = packed;
        }
      }
    }
    __syncthreads();
    NS_STAMP(2);

    // ---- stream: steady-state rounds consume slot i and refill it kPF items ahead with NO conditions inside, so
    //      the compiler emits counted vmcnt waits instead of draining the queue; the last rounds are peeled ----
    const int rounds = nitems / PF, rem = nitems - rounds * PF;
    constexpr int SPR = PF / NQ;  // k-steps per round
    if (full_pipe) {
      int r = 0;
#ifdef NS_TRACE
      {  // first item's arrival: wait for the oldest load only
        asm volatile("" ::"v"(qv[0].x));
        NS_STAMP(3);
      }
#endif
      for (; r + 1 < rounds; r++) {
        NS_FOR_SLOTS({
          // pin the order consume-slot -> refill-slot: hipcc otherwise sinks all refills to the end of the round
          compute(ic, sl0 + (r * SPR + i / NQ) * NW);
          __builtin_amdgcn_sched_barrier(0);
          issue(ic, first + ((r + 1) * SPR + i / NQ) * NW);
          __builtin_amdgcn_sched_barrier(0);
        })
      }
      // last full round: refill only what the remainder needs
      NS_FOR_SLOTS({
        compute(ic, sl0 + (r * SPR + i / NQ) * NW);
        __builtin_amdgcn_sched_barrier(0);
        if (i < rem) issue(ic, first + ((r + 1) * SPR + i / NQ) * NW);
        __builtin_amdgcn_sched_barrier(0);
      })
      r++;
      NS_FOR_SLOTS({
        if (i < rem) compute(ic, sl0 + (r * SPR + i / NQ) * NW);
        __builtin_amdgcn_sched_barrier(0);
      })
    } else {
      NS_FOR_SLOTS({
        if (i < nitems) compute(ic, sl0 + (i / NQ) * NW);
        __builtin_amdgcn_sched_barrier(0);
      })
    }
  }
  NS_STAMP(4);

  // ---- cross-wave reduction through LDS, then epilogue ----
  __syncthreads();
  NS_STAMP(5);
  floatx4* red = reinterpret_cast<floatx4*>(smem);  // [NW][NQ][MB][64]
#pragma unroll
  for (int q = 0; q < NQ; q++)
#pragma unroll
    for (int mb = 0; mb < MB; mb++) red[((w * NQ + q) * MB + mb) * 64 + l] = acc[q][mb];
  __syncthreads();
  if (w < MB) {
    const int mb = w;
    floatx4 sum[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      sum[q] = floatx4{0.f, 0.f, 0.f, 0.f};
      for (int ww = 0; ww < NW; ww++) sum[q] += red[((ww * NQ + q) * MB + mb) * 64 + l];
    }
    const int col = tile * 16 + nn;
    const int ncols = p.n[DUAL ? 0 : seg];
    if (col < ncols) {
      float* cbase = p.c[DUAL ? 0 : seg];
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int row = mb * 16 + 4 * g + rr;
        if (row >= p.m) continue;
        float v = sum[0][rr];
        if constexpr (DUAL) {
          // tmp1 = act(A*W1) ; tmp2 = (A*W3) * tmp1   (ip_fusion_ffn.cpp:364-406)
          const float t1 = (p.epilogue == 5) ? epi_silu(v) : epi_gelu(v);
          if (p.c2) p.c2[size_t(row) * p.ldc + col] = t1;
          v = sum[1][rr] * t1;
        } else {
          const float dv = p.d ? p.d[size_t(row) * p.ldd + col] : 0.f;
          v = epi_apply(v, dv, p.epilogue);
        }
        cbase[size_t(row) * p.ldc + col] = v;
        _Float16* c16 = p.c16[DUAL ? 0 : seg];
        if (c16) c16[size_t(row) * p.ldc + col] = (_Float16)v;
      }
    }
  }
  NS_STAMP(6);
#ifdef NS_TRACE
  if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096)  // where the wave ran: XCC_ID (reg 20) and HW_ID (reg 4)
    p.trace[(size_t(blockIdx.x) * 16 + (threadIdx.x >> 6)) * 8 + 7] =
        (uint64_t(__builtin_amdgcn_s_getreg((31 << 11) | 20)) << 32) | uint32_t(__builtin_amdgcn_s_getreg((31 << 11) | 4));
#endif
}

#ifdef NS_TRACE
static unsigned long long* g_trace_buf = nullptr;
constexpr size_t kTraceBytes = size_t(4096) * 16 * 8 * 8;
unsigned long long* trace_buffer() {
  if (!g_trace_buf) {
    hipMalloc((void**)&g_trace_buf, kTraceBytes);
    hipMemset(g_trace_buf, 0, kTraceBytes);
  }
  return g_trace_buf;
}
}  // namespace ns
extern "C" int ns_hip_debug_trace_read(void* host_dst, size_t bytes) {
  hipDeviceSynchronize();
  const size_t n = bytes < ns::kTraceBytes ? bytes : ns::kTraceBytes;
  if (hipMemcpy(host_dst, ns::trace_buffer(), n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  hipMemset(ns::trace_buffer(), 0, ns::kTraceBytes);
  return 0;
}
namespace ns {
#endif

bool smallm_supported(const ns_weight* w, int m) {
  (void)m;
  const int kstep = w->kstep_len;
  if (w->blocksize >= w->k) return true;
  if (w->blocksize % 32 != 0) return false;
  if (w->blocksize < kstep) return kstep % w->blocksize == 0;
  return w->blocksize % kstep == 0;
}

template <int KIND, int SPS, int SK, bool ASYM>
static hipError_t launch_smallm_k(const SmallMParams& p, bool dual, int mb, int grid, int nw, size_t lds,
                                  hipStream_t st) {
  const dim3 g(grid), b(nw * 64);
  // The 128-VGPR instantiation (4 waves per SIMD, 2-deep ring) is the default for every plain MB == 1 launch: measured
  // +2 % tokens/s over the 168-VGPR / 4-deep one on QKV, WO and lm_head as well as the down projection; the fused
  // gate/up launch measured the same either way and stays on the 168-VGPR variant.
  static const bool narrow_all = getenv("NS_NO_WIDE") != nullptr;  // diagnostics: 168-VGPR variant where possible
  // plain MB == 1 launches have the WIDE instantiation as well, the only one that runs more than 8 waves
  auto go = [&](auto mb_c, auto dual_c) {
    constexpr int MB = mb_c;
    constexpr bool DUAL = dual_c;
    if constexpr (MB == 1 && !DUAL) {
      if (nw > 8 || !narrow_all) {
        hipLaunchKernelGGL((smallm_kernel<KIND, SPS, MB, DUAL, SK, ASYM, true>), g, b, lds, st, p);
        return hipGetLastError();
      }
    }
    if (nw > 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL((smallm_kernel<KIND, SPS, MB, DUAL, SK, ASYM, false>), g, b, lds, st, p);
    return hipGetLastError();
  };
  if (dual && mb == 1) return go(int_c<1>{}, std::true_type{});
  if (mb == 1) return go(int_c<1>{}, std::false_type{});
  if (mb == 2) return go(int_c<2>{}, std::false_type{});
  return go(int_c<4>{}, std::false_type{});
}

// dual (gate/up) launches need MB == 1; callers split larger M into the unfused path
bool smallm_dual_ok(int m) { return m <= 16; }

hipError_t launch_smallm(const SmallMArgs& a, hipStream_t st) {
  if (a.m <= 16) {  // decode / small batches: the shared-activation kernel (ns_gemvs.hip) from two rows on ...
    hipError_t e = launch_gemvs(a, st);
    if (e != hipErrorNotSupported) return e;
    e = launch_gemv(a, st);  // ... the one-tile-per-workgroup streaming kernel (ns_gemv.hip) for single rows
    if (e != hipErrorNotSupported) return e;
  }
  if (a.link || a.rope) return hipErrorNotSupported;  // carried norm / fused RoPE exist only in gemv_kernel: never silently dropped
  const ns_weight* w0 = a.seg[0].w;
  SmallMParams p;
  memset(&p, 0, sizeof(p));
  p.a = a.a;
  p.a16 = static_cast<const _Float16*>(a.a16);
  p.lda = a.lda;
  p.m = a.m;
  p.k = w0->k;
  p.ksteps = w0->ksteps;
  p.nseg = a.nseg;
  int tiles = 0;
  for (int i = 0; i < a.nseg; i++) {
    const ns_weight* w = a.seg[i].w;
    p.tile_begin[i] = tiles;
    tiles += w->ntiles;
    p.codes[i] = w->codes;
    p.scales[i] = w->scales;
    p.zps[i] = w->zps;
    p.codes_bytes[i] = uint32_t(w->codes_bytes);
    p.scales_bytes[i] = uint32_t(w->scales_bytes);
    p.zps_bytes[i] = uint32_t(w->zps_bytes);
    if (w->codes_bytes >= (size_t(1) << 32)) return hipErrorInvalidValue;
    p.c[i] = a.seg[i].c;
    p.c16[i] = static_cast<_Float16*>(a.seg[i].c16);
    p.n[i] = w->n;
  }
  p.tile_begin[a.nseg] = tiles;
  p.ldc = a.ldc;
  p.scale_dt = w0->scale_dt;
  p.qstride = w0->qstride;
  p.sstride = w0->sstride;
  p.zstride = w0->zstride;
#ifdef NS_TRACE
  p.trace = trace_buffer();
#endif
  p.srows = w0->srows;
  if (!srow_params(w0, &p.srow_mul, &p.srow_shift)) return hipErrorInvalidValue;
  p.epilogue = a.epilogue;
  p.d = a.d;
  p.ldd = a.ldd;
  p.c2 = a.c2;
  if (w0->kind == WK_F4) f4_lut_planes(w0->lut, &p.lut);
  p.f8 = f8_consts(w0->qtype);
  static const int env_nw = getenv("NS_NW") ? atoi(getenv("NS_NW")) : 0;  // diagnostics: waves per workgroup

  const int mb = a.m <= 16 ? 1 : (a.m <= 32 ? 2 : 4);
  if (a.dual && mb != 1) return hipErrorInvalidValue;
  const int rows = a.m < 16 * mb ? a.m : 16 * mb;
  const int grid = a.dual ? w0->ntiles : tiles;
  // waves per workgroup: every wave runs a kPF-deep load ring, so what matters is (a) enough waves on the chip to
  // cover bandwidth x latency (~3-4k waves) and (b) as many k-steps per wave as possible so that dequant/MFMA of one
  // step overlaps the loads of the next ones.  Measured on MI355X (profiles/r01*): many tiles -> few waves each.
  int nw = 8;
  if (mb == 1) nw = decode_waves(grid, w0->ksteps, a.dual);  // the same split of K as gemv_kernel's rule (ns_gemv.hip: decode_waves)
  if (env_nw == 8 || env_nw == 4 || env_nw == 2 || (env_nw == 16 && mb == 1)) nw = env_nw;
  static const int env_nw_plain = getenv("NS_NW_PLAIN") ? atoi(getenv("NS_NW_PLAIN")) : 0;  // diagnostics
  if (!a.dual && mb == 1 && (env_nw_plain == 2 || env_nw_plain == 4 || env_nw_plain == 8 || env_nw_plain == 16))
    nw = env_nw_plain;
  // LDS: A chunk (rows x (chunk_k + 8) halves) and the reduction scratch.  The chunk is halved while it is above 64 KiB but never below
  // nw = 8 k-steps, so from 32 rows (4-bit records, kstep 128) / 64 rows (8-bit and fp8, kstep 64) the launch asks for MORE than 64 KiB:
  // 66,048 B at 32 rows and 132,096 B at 64 rows of 4-bit records, 66,560 B at 64 rows of 8-bit ones.  This is a plain launch, not
  // launch_lds: the runtime grants these sizes on gfx950 (160 KiB per workgroup) without the kernel's limit being raised —
  // tests/test_gpu_rows17_64.py pins both crossings (docs/kernels/smallm.md)
  const int kstep = w0->kstep_len;
  int chunk_steps = ((w0->ksteps + nw - 1) / nw) * nw;
  const size_t budget = 64 * 1024;
  while (size_t(rows) * (size_t(chunk_steps) * kstep + 8) * 2 > budget && chunk_steps > nw)
    chunk_steps = ((chunk_steps / 2 + nw - 1) / nw) * nw;
  p.chunk_steps = chunk_steps;
  size_t lds = size_t(rows) * (size_t(chunk_steps) * kstep + 8) * 2;
  const size_t red = size_t(nw) * (a.dual ? 2 : 1) * mb * 64 * 16;
  if (red > lds) lds = red;

  return with_format(w0->kind, w0->sps, w0->scale_dt, w0->asym, [&](auto kind_c, auto sps_c, auto sk_c, auto asym_c) {
    return launch_smallm_k<kind_c, sps_c, sk_c, asym_c>(p, a.dual, mb, grid, nw, lds, st);
  });
}

// ============================================================================================================
// gemm_kernel — prefill / large-M tiled MFMA GEMM: C[M][N] = A[M][K] * dequant(W)
//
// 128 x 128 output tile per 256-thread workgroup (4 waves as 2 x 2, each 64 x 64 = 4 x 4 MFMA 16x16 tiles), one
// k-step (128 k for 4-bit, 64 for 8-bit) per iteration.  The weight tile comes straight from the streaming layout:
// a lane's 16 B ARE the B fragments of k-slot c / column nn, so dequantised codes are written to LDS as
// [tile][j][c][nn][8 halves] and read back as conflict-free ds_read_b128 MFMA operands.  A (fp32 at the boundary)
// is converted to fp16 on the way into LDS.  Group scales are applied to the fp32 MFMA results (same exact
// w = (code - zp) * scale, fp32 accumulate semantics as the decode kernel; reference kernel_ref.h:1027-1127).
// Roofline: MFMA fp16 (2.5 PFLOP/s dense); this first version is single-buffered.
// ============================================================================================================
constexpr int kGemmBM = 128, kGemmTiles = 8;  // 8 column tiles of 16 = 128 columns

struct GemmParams {
  const float* a;
  int lda, m, k, n;
  int ksteps, ntiles;
  const uint4* codes;
  const void* scales;
  const int8_t* zps;
  uint32_t codes_bytes, scales_bytes, zps_bytes;
  uint32_t qstride, sstride, zstride;
  float* c;
  _Float16* c16;  // optional fp16 shadow of C (same ldc)
  int ldc;
  int srows, srow_mul, srow_shift;
  int epilogue;
  const float* d;
  int ldd;
  F4Lut lut;
  F8Consts f8;
};

template <int KIND, int SPS, int SK, bool ASYM>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmParams p) {
  constexpr int NJ = kind_is_8bit(KIND) ? 2 : 4;
  constexpr int KSTEP = NJ * 32;
  constexpr int SBYTES = SPS * (SK == SK_F32 ? 4 : 2);
  constexpr int ASTR = KSTEP + 8;  // halves per A row in LDS (+16 B skews banks)
  using Corr = CorrRaw<SPS, SK, ASYM>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  _Float16* a_lds = reinterpret_cast<_Float16*>(smem);                         // [128][ASTR]
  uint4v* b_lds = reinterpret_cast<uint4v*>(smem + size_t(kGemmBM) * ASTR * 2);  // [8][NJ][4][16] x 16 B

  const int tid = threadIdx.x;
  const int w = tid >> 6, l = tid & 63, nn = l & 15, g = l >> 4;
  const int wm = w >> 1, wn = w & 1;
  const int tile0 = blockIdx.x * kGemmTiles;  // first 16-column tile of this workgroup
  const int row0 = blockIdx.y * kGemmBM;

  const Rsrc rq = make_rsrc(p.codes, p.codes_bytes);
  const Rsrc rs = make_rsrc(p.scales, p.scales_bytes);
  const Rsrc rz = make_rsrc(p.zps, p.zps_bytes);
  const I4Consts i4c = {0x000f000fu, 0x00f000f0u, 0x64006400u};

  floatx4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; mi++)
#pragma unroll
    for (int ni = 0; ni < 4; ni++) acc[mi][ni] = floatx4{0.f, 0.f, 0.f, 0.f};

  for (int s = 0; s < p.ksteps; s++) {
    const uint32_t srow = uint32_t(s * p.srow_mul) >> p.srow_shift;
    // ---- global loads of this k-step: two weight lanes per thread, the compute lanes' scales, 16 float4 of A ----
    uint4v qv[2];
    Corr zc[2];  // zero points ride in the CorrRaw container (scales of the staging lanes are not needed)
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int tl = w + 4 * r;  // tile of the workgroup this wave stages
      const int tile = tile0 + tl;
      const uint32_t soff = (uint32_t(tile) * p.ksteps + s) * p.qstride;
      qv[r] = tile < p.ntiles ? __builtin_bit_cast(uint4v, __builtin_amdgcn_raw_buffer_load_b128(rq, l * 16, soff, 0))
                              : uint4v{0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u};
      if constexpr (ASYM) {
        const uint32_t crow = uint32_t(tile) * p.srows + srow;
        if constexpr (SPS == 4)
          zc[r].z[0] = __builtin_amdgcn_raw_buffer_load_b32(rz, nn * SPS, crow * p.zstride, 0);
        else if constexpr (SPS == 2)
          zc[r].z[0] = __builtin_amdgcn_raw_buffer_load_b16(rz, nn * SPS, crow * p.zstride, 0);
        else
          zc[r].z[0] = __builtin_amdgcn_raw_buffer_load_b8(rz, nn * SPS, crow * p.zstride, 0);
      }
    }
    Corr sc_raw[4];
#pragma unroll
    for (int ni = 0; ni < 4; ni++) {
      const int tile = tile0 + wn * 4 + ni;
      const uint32_t crow = uint32_t(tile) * p.srows + srow;
      corr_issue<SPS, SK, false>(rs, rz, nn * SBYTES, 0, crow * p.sstride, 0, reinterpret_cast<CorrRaw<SPS, SK, false>&>(sc_raw[ni]));
    }
    // ---- A tile: fp32 -> fp16 -> LDS ----
    __syncthreads();  // previous iteration's MFMAs are done with LDS
    {
      constexpr int QPR = KSTEP / 4;  // float4 per row
      const bool vec_ok = ((p.lda & 3) == 0) && ((reinterpret_cast<uintptr_t>(p.a) & 15) == 0);
#pragma unroll 4
      for (int idx = tid; idx < kGemmBM * QPR; idx += 256) {
        const int r = idx / QPR, kq = (idx % QPR) * 4;
        const int row = row0 + r, gk = s * KSTEP + kq;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < p.m) {
          const float* src = p.a + size_t(row) * p.lda + gk;
          if (vec_ok && gk + 3 < p.k) {
            v = *reinterpret_cast<const float4*>(src);
          } else {
            if (gk + 0 < p.k) v.x = src[0];
            if (gk + 1 < p.k) v.y = src[1];
            if (gk + 2 < p.k) v.z = src[2];
            if (gk + 3 < p.k) v.w = src[3];
          }
        }
        half2_t h0 = {(_Float16)v.x, (_Float16)v.y}, h1 = {(_Float16)v.z, (_Float16)v.w};
        *reinterpret_cast<uint2*>(a_lds + r * ASTR + kq) = uint2{as_u32(h0), as_u32(h1)};
      }
    }
    // ---- B tile: dequantise (code - zp), exact in fp16, straight into MFMA fragment order ----
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int tl = w + 4 * r;
      const uint32_t xw[4] = {qv[r].x, qv[r].y, qv[r].z, qv[r].w};
#pragma unroll
      for (int j = 0; j < NJ; j++) {
        float zp = 0.f;
        if constexpr (ASYM) zp = float(int(int8_t((zc[r].z[0] >> (8 * ((j * SPS) / NJ))) & 0xff)));
        half8_t b;
        if constexpr (KIND == WK_INT4) {
          const _Float16 zl = (_Float16)(-1032.f - zp), zh = (_Float16)(-72.f - zp);
          b = cvt_i4x8(xw[j], i4c, half2_t{zl, zl}, half2_t{zh, zh});
        } else if constexpr (KIND == WK_INT8) {
          const _Float16 zo = (_Float16)(-1152.f - zp);
          b = cvt_i8x8(xw[2 * j], xw[2 * j + 1], half2_t{zo, zo});
        } else if constexpr (KIND == WK_F8) {
          b = cvt_f8x8(xw[2 * j], xw[2 * j + 1], p.f8);
        } else {
          b = cvt_f4x8(xw[j], p.lut);
        }
        b_lds[((tl * NJ + j) * 4 + g) * 16 + nn] = __builtin_bit_cast(uint4v, b);
      }
    }
    float sc[4][4];
#pragma unroll
    for (int ni = 0; ni < 4; ni++) {
      float zz[4];
      corr_decode<SPS, SK, false, NJ>(reinterpret_cast<CorrRaw<SPS, SK, false>&>(sc_raw[ni]), sc[ni], zz);
    }
    __syncthreads();
    // ---- MFMA: 4 x 4 tiles x NJ k-slices per wave ----
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      half8_t af[4], bf[4];
#pragma unroll
      for (int mi = 0; mi < 4; mi++)
        af[mi] = *reinterpret_cast<const half8_t*>(a_lds + (wm * 64 + mi * 16 + nn) * ASTR + 32 * j + 8 * g);
#pragma unroll
      for (int ni = 0; ni < 4; ni++)
        bf[ni] = __builtin_bit_cast(half8_t, b_lds[(((wn * 4 + ni) * NJ + j) * 4 + g) * 16 + nn]);
#pragma unroll
      for (int mi = 0; mi < 4; mi++)
#pragma unroll
        for (int ni = 0; ni < 4; ni++) {
          const floatx4 dd = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mi], bf[ni], floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          acc[mi][ni] += dd * sc[ni][j];
        }
    }
  }
  // ---- epilogue ----
#pragma unroll
  for (int mi = 0; mi < 4; mi++)
#pragma unroll
    for (int ni = 0; ni < 4; ni++) {
      const int col = (tile0 + wn * 4 + ni) * 16 + nn;
      if (col >= p.n) continue;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = row0 + wm * 64 + mi * 16 + 4 * g + r;
        if (row >= p.m) continue;
        float v = acc[mi][ni][r];
        const float dv = p.d ? p.d[size_t(row) * p.ldd + col] : 0.f;
        v = epi_apply(v, dv, p.epilogue);
        p.c[size_t(row) * p.ldc + col] = v;
        if (p.c16) p.c16[size_t(row) * p.ldc + col] = (_Float16)v;
      }
    }
}

hipError_t launch_gemm(const SmallMArgs& a, hipStream_t st) {
  {
    const hipError_t e = launch_gemm2(a, st);
    if (e != hipErrorNotSupported) return e;
  }
  const ns_weight* w0 = a.seg[0].w;
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.a = a.a;
  p.lda = a.lda;
  p.m = a.m;
  p.k = w0->k;
  p.n = w0->n;
  p.ksteps = w0->ksteps;
  p.ntiles = w0->ntiles;
  p.codes = w0->codes;
  p.scales = w0->scales;
  p.zps = w0->zps;
  p.codes_bytes = uint32_t(w0->codes_bytes);
  p.scales_bytes = uint32_t(w0->scales_bytes);
  p.zps_bytes = uint32_t(w0->zps_bytes);
  p.qstride = w0->qstride;
  p.sstride = w0->sstride;
  p.zstride = w0->zstride;
  p.c = a.seg[0].c;
  p.c16 = static_cast<_Float16*>(a.seg[0].c16);  // the fp16 shadow of C: the same value, rounded once more (C does not depend on it)
  p.ldc = a.ldc;
  p.srows = w0->srows;
  if (!srow_params(w0, &p.srow_mul, &p.srow_shift)) return hipErrorInvalidValue;
  p.epilogue = a.epilogue;
  p.d = a.d;
  p.ldd = a.ldd;
  if (w0->kind == WK_F4) f4_lut_planes(w0->lut, &p.lut);
  p.f8 = f8_consts(w0->qtype);
  const int kstep = w0->kstep_len;
  const dim3 grid((w0->ntiles + kGemmTiles - 1) / kGemmTiles, (a.m + kGemmBM - 1) / kGemmBM);
  const size_t lds = size_t(kGemmBM) * (kstep + 8) * 2 + size_t(kGemmTiles) * kstep * 16 * 2;
  return with_format(w0->kind, w0->sps, w0->scale_dt, w0->asym, [&](auto kind_c, auto sps_c, auto sk_c, auto asym_c) {
    hipLaunchKernelGGL((gemm_kernel<kind_c, sps_c, sk_c, asym_c>), grid, dim3(256), lds, st, p);
    return hipGetLastError();
  });
}

// ============================================================================================================
// unpack: device layout -> fp32 [K][N]   (BTLAGemmUnPackB semantics: w = (code - zp) * scale / LUT[code] * scale)
// ============================================================================================================
struct Lut16 {
  float v[16];
};
__global__ void unpack_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                              const uint8_t* __restrict__ zps, uint32_t qstride, uint32_t sstride, uint32_t zstride,
                              float* __restrict__ out, int ld, int n, int k, int ksteps,
                              int kind, int sps, int srows, int num, int den, uint32_t scale_dt, Lut16 lut,
                              uint32_t qtype) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gid >= size_t(n) * k) return;
  const int col = int(gid % n);
  const int kk = int(gid / n);
  const int t = col >> 4, nn = col & 15;
  const int kstep = kind_is_8bit(kind) ? 64 : 128;
  const int s = kk / kstep, r = kk % kstep;
  const int j = r >> 5, c = (r >> 3) & 3, i = r & 7;
  const uint32_t* lane_words =
      reinterpret_cast<const uint32_t*>(codes + (size_t(t) * ksteps + s) * qstride + size_t(c * 16 + nn) * 16);
  const int nj = kind_is_8bit(kind) ? 2 : 4;
  const int srow = (s * num) / den;
  const size_t crow = size_t(t) * srows + srow;
  const size_t cidx = size_t(nn) * sps + (j * sps) / nj;
  const float sc = load_scale(scales + crow * sstride, cidx, scale_dt);
  const int zp = zps ? int(int8_t(zps[crow * zstride + cidx])) : 0;
  float v;
  if (kind == WK_INT8) {
    const uint32_t word = lane_words[2 * j + (i >> 2)];
    v = float(int(int8_t((word >> (8 * (i & 3))) & 0xff)) - zp);
  } else if (kind == WK_F8) {  // f8_to_fp32, kernel_ref.h:984-1002
    const uint32_t code = (lane_words[2 * j + (i >> 2)] >> (8 * (i & 3))) & 0xff;
    const int ebits = qtype == DT_F8_E4M3 ? 4 : 5, mbits = 7 - ebits;
    const uint32_t e = ((code & 0x7f) >> mbits) - (1u << (ebits - 1)) + 1 + 127;
    v = __uint_as_float(((code << 24) & 0x80000000u) | (e << 23) | ((code << (23 - mbits)) & 0x007fffffu));
  } else {
    const int u = (lane_words[j] >> nib_shift(i)) & 0xf;
    v = (kind == WK_INT4) ? float(u - 8 - zp) : lut.v[u];
  }
  out[size_t(kk) * ld + col] = v * sc;
}

hipError_t launch_unpack_fp32(const ns_weight* w, float* out, int ld, hipStream_t st) {
  Lut16 lut;
  for (int i = 0; i < 16; i++) lut.v[i] = w->lutf[i];
  int num, den;
  srow_rule(w, &num, &den);
  const size_t total = size_t(w->n) * w->k;
  hipLaunchKernelGGL(unpack_kernel, dim3((total + 255) / 256), dim3(256), 0, st, (const uint8_t*)w->codes,
                     (const uint8_t*)w->scales, (const uint8_t*)w->zps, w->qstride, w->sstride, w->zstride, out, ld, w->n,
                     w->k, w->ksteps, w->kind, w->sps, w->srows, num, den, w->scale_dt, lut, w->qtype);
  return hipGetLastError();
}

// ---- weight prefetch ------------------------------------------------------------------------------------------------
// Reads a span of a weight's streaming buffer with default-policy loads and throws the data away: the lines land in the
// die-level Infinity Cache (256 MiB), so a decode launch that follows finds (part of) its stream there instead of in
// HBM.  Meant to run on a second stream / graph branch beside the PREVIOUS GEMV of the chain, whose ramp-up and tail
// leave HBM idle.  Few workgroups, eight 16-byte loads in flight per lane.
__global__ __launch_bounds__(256) void prefetch_kernel(const uint4v* __restrict__ p, size_t n16, uint32_t* __restrict__ sink) {
  const size_t stride = size_t(gridDim.x) * blockDim.x;
  uint32_t acc = 0;
  for (size_t idx = size_t(blockIdx.x) * blockDim.x + threadIdx.x; idx < n16; idx += 8 * stride) {
    uint4v v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const size_t j = idx + i * stride;
      v[i] = j < n16 ? p[j] : uint4v{0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < 8; i++) acc |= v[i].x & v[i].w;
  }
  // never true for real data in both words of every line; keeps the loads alive without a store in practice
  if (acc == 0xdeadbeefu && sink) sink[0] = acc;
}
hipError_t launch_prefetch(const ns_weight* w, size_t offset, size_t bytes, int grid, hipStream_t st) {
  const size_t span = w->alloc_bytes;
  offset &= ~size_t(15);
  if (offset >= span) return hipSuccess;
  bytes = std::min(bytes, span - offset) & ~size_t(15);
  if (!bytes) return hipSuccess;
  if (grid <= 0) grid = 64;
  grid = std::min(grid, 4096);
  const uint4v* p = reinterpret_cast<const uint4v*>(reinterpret_cast<const unsigned char*>(w->codes) + offset);
  hipLaunchKernelGGL(prefetch_kernel, dim3(grid), dim3(256), 0, st, p, bytes / 16, static_cast<uint32_t*>(nullptr));
  return hipGetLastError();
}

}  // namespace ns
