// ns_moe_loop.hip — the per-row loop kernel of ns_hip_mul_mat_id, the server that takes every call: one workgroup per (column tile, token
// row) looks its row's expert up in the group's device table and streams that expert's tile (numerics: docs/kernels/other.md, section 4.7).
#include <hip/hip_runtime.h>

#include "ns_dev.h"
#include "ns_moe.h"

namespace ns {
namespace {
constexpr int kMoeWaves = 8, kMoeThreads = kMoeWaves * 64;

// the reference's fp8 value of a code (f8_to_fp32, kernel_ref.h:984-1002): +-2^(e - bias) * (1 + m / 2^mbits) for EVERY code
__device__ __forceinline__ float moe_f8_value(uint32_t code, int e5m2) {
  const int mbits = e5m2 ? 2 : 3, bias = e5m2 ? 15 : 7;
  const int e = int((code & 0x7fu) >> mbits), m = int(code & ((1u << mbits) - 1u));
  const float v = ldexpf(1.f + float(m) / float(1 << mbits), e - bias);
  return (code & 0x80u) ? -v : v;
}

template <int KIND>  // WK_INT4, WK_INT8, WK_F4 or WK_F8
__global__ __launch_bounds__(kMoeThreads) void moe_gemv_kernel(const MoeParams p) {
  constexpr int NJ = kind_is_8bit(KIND) ? 2 : 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char moe_smem[];
  __shared__ float red[kMoeWaves][16];
  __shared__ float lut_s[16];
  _Float16* a_lds = reinterpret_cast<_Float16*>(moe_smem);  // the token row, rounded to fp16 like every default kernel
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, nn = l & 15, cslot = l >> 4;
  const int tile = blockIdx.x, row = blockIdx.y;
  const int32_t e_id = p.ids[size_t(row) * p.ids_stride + p.id];
  const bool valid = e_id >= 0 && e_id < p.n_as;  // the reference asserts this (:7860); here the row is zeroed
  const MoeExpertRow ex = p.table[valid ? e_id : 0];
  const int kpad = p.ksteps * p.kstep_len;
  for (int i = tid; i < kpad; i += kMoeThreads) a_lds[i] = i < p.k ? (_Float16)p.a[size_t(row) * p.lda + i] : (_Float16)0.f;
  if (KIND == WK_F4 && tid < 16) lut_s[tid] = p.lut[tid];
  __syncthreads();
  const int sbytes = p.scale_dt == DT_F32 ? 4 : 2;
  const int rec_sbytes = p.sps * sbytes;
  struct Corr {
    uint32_t s[4];
    uint32_t z;
  };
  auto fetch_corr = [&](int s) {
    Corr c{{0, 0, 0, 0}, 0};
    const uint32_t srow = uint32_t(s * p.srow_mul) >> p.srow_shift;
    const size_t crow = size_t(tile) * p.srows + srow;
    const uint8_t* sp = ex.scales + crow * p.sstride + size_t(nn) * rec_sbytes;
    if (rec_sbytes == 16) {
      const uint4v v = *reinterpret_cast<const uint4v*>(sp);
      c.s[0] = v.x, c.s[1] = v.y, c.s[2] = v.z, c.s[3] = v.w;
    } else if (rec_sbytes == 8) {
      const uint2 v = *reinterpret_cast<const uint2*>(sp);
      c.s[0] = v.x, c.s[1] = v.y;
    } else if (rec_sbytes == 4) {
      c.s[0] = *reinterpret_cast<const uint32_t*>(sp);
    } else {
      c.s[0] = *reinterpret_cast<const uint16_t*>(sp);
    }
    if (p.asym) {
      const int8_t* zp = ex.zps + crow * p.zstride + nn * p.sps;
      for (int e = 0; e < p.sps; e++) c.z |= uint32_t(uint8_t(zp[e])) << (8 * e);
    }
    return c;
  };
  float acc = 0.f;
  auto consume = [&](const uint4v& rec, const Corr& cr, int s) {
    const uint32_t xw[4] = {rec.x, rec.y, rec.z, rec.w};
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const int e = (j * p.sps) / NJ;
      auto pick = [&](int i) { return i == 0 ? cr.s[0] : (i == 1 ? cr.s[1] : (i == 2 ? cr.s[2] : cr.s[3])); };
      float sb;
      if (p.scale_dt == DT_F32) {
        sb = __builtin_bit_cast(float, pick(e));
      } else {
        const uint32_t h = (pick(e >> 1) >> (16 * (e & 1))) & 0xffffu;
        sb = p.scale_dt == DT_BF16 ? __builtin_bit_cast(float, h << 16) : f16_bits_to_f32(h);
      }
      const float zb = p.asym ? float(int(int8_t((cr.z >> (8 * e)) & 0xffu))) : 0.f;
      const half8_t av = *reinterpret_cast<const half8_t*>(a_lds + s * p.kstep_len + 32 * j + 8 * cslot);
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        float wv;
        if constexpr (KIND == WK_INT8) {
          const uint32_t word = i < 4 ? xw[2 * j] : xw[2 * j + 1];
          wv = float(int(int8_t((word >> (8 * (i & 3))) & 255u))) - zb;
        } else if constexpr (KIND == WK_F8) {
          const uint32_t word = i < 4 ? xw[2 * j] : xw[2 * j + 1];
          wv = moe_f8_value((word >> (8 * (i & 3))) & 255u, p.f8_e5m2);
        } else {
          const uint32_t code = (xw[j] >> (((i & 1) << 4) + ((i >> 1) << 2))) & 15u;  // nibble i at bit {0,16,4,20,...}
          if constexpr (KIND == WK_F4)
            wv = lut_s[code];
          else
            wv = float(int(code) - 8) - zb;
        }
        dot = fmaf(float(av[i]), wv, dot);
      }
      acc = fmaf(dot, sb, acc);
    }
  };
  auto load_rec = [&](int s) {
    return *reinterpret_cast<const uint4v*>(ex.codes + (size_t(tile) * p.ksteps + s) * p.qstride + l * 16);
  };
  if (valid) {
    for (int s = w; s < p.ksteps; s += 4 * kMoeWaves) {
      uint4v rec[4];
      Corr cr[4];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int st = s + t * kMoeWaves;
        const bool on = st < p.ksteps;
        rec[t] = on ? load_rec(st) : uint4v{0, 0, 0, 0};
        cr[t] = on ? fetch_corr(st) : Corr{{0, 0, 0, 0}, 0};
      }
#pragma unroll
      for (int t = 0; t < 4; t++)
        if (s + t * kMoeWaves < p.ksteps) consume(rec[t], cr[t], s + t * kMoeWaves);
    }
  }
  acc += __shfl_xor(acc, 16);
  acc += __shfl_xor(acc, 32);
  if (l < 16) red[w][l] = acc;
  __syncthreads();
  if (tid < 16) {
    const int col = tile * 16 + tid;
    if (col < p.n) {
      float v = 0.f;
#pragma unroll
      for (int ww = 0; ww < kMoeWaves; ww++) v += red[ww][tid];
      const float dv = p.d ? p.d[size_t(row) * p.ldd + col] : 0.f;
      v = epi_apply(v, dv, p.epilogue);
      p.c[size_t(row) * p.ldc + col] = v;
    }
  }
}

}  // namespace

hipError_t launch_moe_loop(const MoeParams& p, int ntiles, hipStream_t st) {
  const dim3 grid(ntiles, p.m), block(kMoeThreads);
  const size_t lds = size_t(p.ksteps) * p.kstep_len * 2;
  if (p.kind == WK_INT8)
    hipLaunchKernelGGL(moe_gemv_kernel<WK_INT8>, grid, block, lds, st, p);
  else if (p.kind == WK_F8)
    hipLaunchKernelGGL(moe_gemv_kernel<WK_F8>, grid, block, lds, st, p);
  else if (p.kind == WK_F4)
    hipLaunchKernelGGL(moe_gemv_kernel<WK_F4>, grid, block, lds, st, p);
  else
    hipLaunchKernelGGL(moe_gemv_kernel<WK_INT4>, grid, block, lds, st, p);
  return hipGetLastError();
}

}  // namespace ns
