// ns_moe.hip — expert-indexed matmul with the routing ON THE DEVICE
//
// Reference: ne_compute_forward_mul_mat_id_q_f32_bestla (/root/reference/neural_speed/core/ne_layers.c:7783-7916): for
// every token row t of src1, `row_id = ids[t][id]` selects one of `n_as` expert blobs and
//       dst[t] = src1[t] . W[row_id]
// is computed by one `bestla_f32f32_forward(row, expert blob, dst row, 1, ...)` call per (token, expert) after the HOST
// has read the ids and grouped the rows (`matrix_rows`, :7855-7866).  That host round trip is what a device-resident,
// graph-captured decode step cannot afford (the ids are the output of the router's top-k on the device), so here the
// kernel itself reads the id: grid = (column tiles, token rows), each workgroup looks up its row's expert in a device
// table of weight descriptors and streams that expert's tile.  The host-pointer surface keeps working unchanged through
// bestla_f32f32_forward; this entry is its device twin.
//
// Numerics: the default semantics of this library — fp16-rounded activations, w = (code - zp) * scale (or LUT[code] *
// scale for the 4-bit float types), fp32 accumulation — evaluated with VALU FMAs: a token row is an M = 1 product, the
// matrix cores have nothing to add and the kernel is bound by the expert's weight stream.  First version: plain
// streaming loop with four records in flight per wave, not tuned like smallm_kernel.
//
// Around that operator, the rest of a Mixtral-style layer's MoE block (docs/kernels/other.md, "MoE decode block"): ns_hip_moe_route, the
// router's soft_max -> top_k -> weights tail in one launch (moe_route_kernel), and ns_hip_moe_ffn_silu, the expert feed-forward block of all
// rows and selections in 1 + n_used launches of the decode kernel (ns_gemv.hip, XV = 4) or, outside their envelope, as the composition of
// ns_hip_mul_mat_id calls with moe_weighted_add_kernel.  At prompt size the block is ONE grouped pass over all (row, selection) pairs
// (moe_ffn_grouped: ns_moe_plan.cpp lays the pairs out, moe_pair_gather_kernel and moe_pair_combine_kernel around the tiled GEMM's launches);
// ns_hip_moe_ffn_gelu is the same block with gelu(gate) * up, ns_hip_moe_route_f the router with the un-normalised weights of the Grok graph.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ns_bestla.h"
#include "ns_api_int.h"
#include "ns_common.h"
#include "ns_dev.h"
#include "ns_moe_plan.h"

namespace ns {
namespace {

constexpr int kMoeWaves = 8, kMoeThreads = kMoeWaves * 64;

struct MoeExpert {  // one row of the device table
  const uint8_t* codes;
  const uint8_t* scales;
  const int8_t* zps;
};

struct MoeParams {
  const MoeExpert* table;
  int n_as;
  const int32_t* ids;
  int ids_stride, id;
  uint32_t qstride, sstride, zstride;
  int ksteps, kstep_len, kind;
  int sps, srows, srow_mul, srow_shift;
  uint32_t scale_dt;
  int asym;
  int n, k, m;
  const float* a;
  int lda;
  float* c;
  int ldc;
  int epilogue;
  const float* d;
  int ldd;
  float lut[16];  // 4-bit float types: code -> value
  int f8_e5m2;    // fp8 codes: 1 = E5M2, 0 = E4M3
};

// ---- prefill size (round 5): the token rows grouped by expert, ONE tiled GEMM per expert over its rows ----------------------------
// The per-row kernels below let every token stream its whole expert: 2048 tokens x 2 experts of a Mixtral layer read 2048 x 29 MB per
// matrix.  The reference groups the rows on the host too (`matrix_rows`, ne_layers.c:7855-7866) and then still calls one
// bestla_f32f32_forward per row; here the id column comes back to the host once (m ints), the rows are gathered in expert order as the
// fp16 operand the tiled GEMM multiplies anyway, every expert's rows are ONE gemm3_kernel launch, and a scatter kernel applies the
// epilogue per token row.  Not capturable (the host reads the ids): a capturing stream keeps the per-row form.
__global__ void moe_ids_column_kernel(const int32_t* __restrict__ ids, int ids_stride, int id, int m, int32_t* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < m) out[t] = ids[size_t(t) * ids_stride + id];
}
__global__ void moe_gather_rows_kernel(const float* __restrict__ a, int lda, const int32_t* __restrict__ perm, int rows, int k, int kpad,
                                       _Float16* __restrict__ out) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;  // one thread per 8 columns
  const int per_row = kpad / 8;
  if (gid >= size_t(rows) * per_row) return;
  const int j = int(gid / per_row), c = int(gid % per_row) * 8;
  const float* src = a + size_t(perm[j]) * lda + c;
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  h8 v;
#pragma unroll
  for (int e = 0; e < 8; e++) v[e] = c + e < k ? (_Float16)src[e] : (_Float16)0.f;
  *reinterpret_cast<h8*>(out + size_t(j) * kpad + c) = v;
}
__global__ void moe_scatter_epilogue_kernel(const float* __restrict__ cg, const int32_t* __restrict__ perm, const int32_t* __restrict__ valid, int rows,
                                            int n, float* __restrict__ c, int ldc, int epilogue, const float* __restrict__ d, int ldd) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gid >= size_t(rows) * n) return;
  const int j = int(gid / n), col = int(gid % n);
  const int t = perm[j];
  float v = valid[j] ? cg[size_t(j) * n + col] : 0.f;  // an id outside the group: a zero product (the per-row kernels do the same)
  const float dv = d ? d[size_t(t) * ldd + col] : 0.f;
  v = epi_apply(v, dv, epilogue);
  c[size_t(t) * ldc + col] = v;
}

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
  const MoeExpert ex = p.table[valid ? e_id : 0];
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

// ---- the router's tail (ns_hip_moe_route): soft_max -> top_k -> get_rows -> sum_rows -> div of the reference graph in one launch ----
// One wave per token row, lane e holds expert e (n_expert <= 64).  The arithmetic is the reference's operation by operation
// (ne_compute_forward_soft_max_f32, ne_layers.c:8887-8954): fp16(x - max) looked up in table_exp_f16, the values summed in double (at most
// 64 fp16 values: exact, so the butterfly's order does not matter), float(1.0 / sum) multiplied in fp32; the selected probabilities summed in
// double in selection order, the sum stored as float (sum_rows) and divided in fp32 (ne_vec_div_f32).  Selection: n_used rounds of a wave-wide
// arg-max on (probability, lower index first) — the reference's std::sort leaves ties unspecified, here the lower expert index wins.
constexpr int kRouteWaves = 4;
__global__ __launch_bounds__(kRouteWaves * 64) void moe_route_kernel(const float* __restrict__ logits, int ld, int m, int n_expert, int n_used,
                                                                     const uint16_t* __restrict__ exp_table, int32_t* __restrict__ ids, int ids_stride,
                                                                     float* __restrict__ weights, int w_stride, float* __restrict__ probs, int raw) {
  const int row = blockIdx.x * kRouteWaves + int(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= m) return;  // (wave-uniform)
  const bool on = lane < n_expert;
  const float ninf = -__builtin_inff();
  const float x = on ? logits[size_t(row) * ld + lane] : ninf;
  float mx = x;  // ne_vec_max_f32
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float y = __shfl_xor(mx, o, 64);
    mx = y > mx ? y : mx;
  }
  float val = 0.f;
  if (on && x != ninf) {
    const _Float16 h = (_Float16)__fsub_rn(x, mx);  // NE_FP32_TO_FP16: round to nearest even
    val = f16_bits_to_f32(exp_table[__builtin_bit_cast(unsigned short, h)]);
  }
  double sum = double(val);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (mx == ninf) sum = double(n_expert);  // (all logits -inf: the reference's start value; every probability is 0)
  const float inv = float(1.0 / sum);
  const float pr = __fmul_rn(val, inv);  // ne_vec_scale_f32
  if (probs && on) probs[size_t(row) * ld + lane] = pr;
  // top-k: key = (probability bits, 63 - lane) — non-negative floats order like their bits; a NaN (outside the contract) counts as 0,
  // lanes beyond n_expert and lanes already taken as -1, so the ids are distinct and in range whatever the row holds
  long long key = on ? ((long long)(pr != pr ? 0u : (__builtin_bit_cast(uint32_t, pr) & 0x7fffffffu)) << 32) | (long long)(63 - lane) : -1ll;
  int my_id = 0;
  float my_p = 0.f;
  for (int r = 0; r < n_used; r++) {
    long long best = key;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long y = __shfl_xor(best, o, 64);
      best = y > best ? y : best;
    }
    const int win = 63 - int(best & 63);
    const float pw = __shfl(pr, win, 64);
    if (lane == r) my_id = win, my_p = pw;
    if (lane == win) key = -1ll;
  }
  double wsum = 0.0;  // sum_rows: double accumulator, in selection order
  for (int r = 0; r < n_used; r++) wsum += double(__shfl(my_p, r, 64));
  const float wsf = float(wsum);
  if (lane < n_used) {
    ids[size_t(row) * ids_stride + lane] = my_id;
    weights[size_t(row) * w_stride + lane] = raw ? my_p : __fdiv_rn(my_p, wsf);  // (raw: grok.cpp:293-299, no sum_rows / div)
  }
}

// the composition's tail (ns_hip_moe_ffn_silu outside the fused launches): out = (first ? 0 : out) + w[t][sel] * x — mul(weights) and add of
// llama.cpp:669-679
__global__ void moe_weighted_add_kernel(float* __restrict__ out, int ldo, const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                        int w_stride, int m, int n, int first) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gid >= size_t(m) * n) return;
  const int t = int(gid / n), col = int(gid % n);
  const float v = (w ? w[size_t(t) * w_stride] : 1.f) * x[size_t(t) * ldx + col];
  float* o = out + size_t(t) * ldo + col;
  *o = first ? v : *o + v;
}

// ---- the block's grouped pass (moe_ffn_grouped): the two memory-bound launches around the tiled GEMM's ----------------------------------------
// gather: fp32 token rows -> fp16 rows [rows][k] in group order (MoePairPlan::src_row; a row selected twice is written twice, src_row < 0 is
// the padding row: zeros).  One thread per 8 columns (k is a multiple of 64): two 16-byte loads where lda and the base allow (vec), one
// 16-byte store.
__global__ void moe_pair_gather_kernel(const float* __restrict__ a, int lda, const int32_t* __restrict__ src_row, int rows, int k, int vec,
                                       _Float16* __restrict__ out) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int per_row = k / 8;
  if (gid >= size_t(rows) * per_row) return;
  const int j = int(gid / per_row), c = int(gid % per_row) * 8;
  const int t = src_row[j];
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  h8 v;
  if (t < 0) {
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = (_Float16)0.f;
  } else {
    const float* src = a + size_t(t) * lda + c;
    float x[8];
    if (vec) {
      const float4 x0 = *reinterpret_cast<const float4*>(src), x1 = *reinterpret_cast<const float4*>(src + 4);
      x[0] = x0.x, x[1] = x0.y, x[2] = x0.z, x[3] = x0.w, x[4] = x1.x, x[5] = x1.y, x[6] = x1.z, x[7] = x1.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++) x[e] = src[e];
    }
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = (_Float16)x[e];
  }
  *reinterpret_cast<h8*>(out + size_t(j) * k + c) = v;
}
// combine: out[t] = sum_i w[t][i] * y[pos(t, i)] — each product rounded, then added, in selection order, starting from the first good
// selection's product (no FMA: the sum does not depend on how the compiler contracts it); pos < 0 (an id outside the groups) contributes
// nothing, a row without a good selection is 0.0f.  One thread per 4 columns of a token row: 16-byte loads of y when n is a multiple of 4,
// 16-byte stores when ldo and the base allow as well (vec_out); nothing is written beyond column n.
__global__ void moe_pair_combine_kernel(const float* __restrict__ y, const int32_t* __restrict__ pos, const float* __restrict__ w, int w_stride, int m,
                                        int n_used, int n, float* __restrict__ out, int ldo, int vec_out) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int per_row = (n + 3) / 4;
  if (gid >= size_t(m) * per_row) return;
  const int t = int(gid / per_row), c = int(gid % per_row) * 4;
  const bool full = (n & 3) == 0;  // (then c + 3 < n and every row of y starts on a 16-byte boundary)
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  bool first = true;
  for (int i = 0; i < n_used; i++) {
    const int j = pos[size_t(t) * n_used + i];
    if (j < 0) continue;
    const float wv = w ? w[size_t(t) * w_stride + i] : 1.f;
    const float* yr = y + size_t(j) * n + c;
    float x[4];
    if (full) {
      const float4 v = *reinterpret_cast<const float4*>(yr);
      x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; e++) x[e] = c + e < n ? yr[e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float v = __fmul_rn(wv, x[e]);
      acc[e] = first ? v : __fadd_rn(acc[e], v);
    }
    first = false;
  }
  float* o = out + size_t(t) * ldo + c;
  if (full && vec_out) {
    *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (c + e < n) o[e] = acc[e];
  }
}

}  // namespace
}  // namespace ns

struct ns_expert_group {
  std::vector<const ns_weight*> experts;
  ns::MoeExpert* table = nullptr;  // device
};

using namespace ns;

namespace ns {
// row thresholds of ns_hip_mul_mat_id's three paths (ns_hip_set_tuning "moe_gemv_rows" / "moe_grouped_rows"): 0 = the environment variable
// if set, else the built-in value; negative = that path is off
static std::atomic<int> g_moe_gemv_rows{0}, g_moe_grouped_rows{0};
void set_moe_tuning(int what, int value) { (what == 0 ? g_moe_gemv_rows : g_moe_grouped_rows).store(value); }
// calls served by [0] the grouped path, [1] the decode kernel, [2] the loop kernel; [3] grouped attempts that returned "not taken" (ns_hip_moe_stats)
static std::atomic<uint64_t> g_moe_stats[4];

// ns_hip_moe_ffn_silu / _gelu: "moe_ffn_fused" (-1 = default: on), "moe_ffn_grouped_rows" (0 = NS_MOE_GROUPED_ROWS if set, else 32; negative =
// never) and the counters (ns_hip_moe_ffn_stats)
static std::atomic<int> g_moe_ffn_fused{-1};
void set_moe_ffn_fused(int on) { g_moe_ffn_fused.store(on < 0 ? -1 : (on != 0)); }
static std::atomic<int> g_moe_ffn_grouped_rows{0};
void set_moe_ffn_grouped_rows(int rows) { g_moe_ffn_grouped_rows.store(rows); }
static std::atomic<uint64_t> g_moe_ffn_stats[4];

// the router's exponential table: table_exp_f16 of the reference (ne_layers.c:745), fp16(expf(fp16 -> fp32(code))) for every code, made by
// the HOST's expf like the reference's and uploaded once per device
static uint16_t f32_to_f16_bits(float f) {  // round to nearest even, subnormals kept (what F16C's conversion and ne_compute_fp32_to_fp16 do)
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x7f800000u) return uint16_t(sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));
  if (x >= 0x477ff000u) return uint16_t(sign | 0x7c00u);  // rounds to 65536 and beyond
  if (x < 0x38800000u) {                                   // below 2^-14: a subnormal half, in units of 2^-24
    if (x < 0x33000000u) return uint16_t(sign);          // below 2^-25: zero (2^-25 itself is a tie to even = zero)
    const int e = int(x >> 23);                           // 102 .. 112
    const uint32_t man = (x & 0x7fffffu) | 0x800000u;     // value = man * 2^(e - 150)
    const int shift = 126 - e;                            // half units: man >> shift
    uint32_t h = man >> shift;
    const uint32_t rem = man & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
    if (rem > halfway || (rem == halfway && (h & 1u))) h++;
    return uint16_t(sign | h);
  }
  uint32_t h = ((x - 0x38000000u) >> 13);
  const uint32_t rem = x & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;
  return uint16_t(sign | h);
}
static float f16_bits_to_f32_host(uint16_t h) {
  const uint32_t sign = uint32_t(h & 0x8000u) << 16, e = (h >> 10) & 31u, man = h & 0x3ffu;
  uint32_t x;
  if (e == 31u) {
    x = sign | 0x7f800000u | (man << 13);
  } else if (e) {
    x = sign | ((e + 112u) << 23) | (man << 13);
  } else {
    float f = float(man) * 5.9604644775390625e-8f;  // man * 2^-24, exact
    memcpy(&x, &f, 4);
    x |= sign;
  }
  float f;
  memcpy(&f, &x, 4);
  return f;
}
static std::mutex g_exp_table_mutex;
static uint16_t* g_exp_table[64];
const uint16_t* moe_exp_table(bool build) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    (void)hipGetLastError();
    set_error("moe_route: no current device for the exponential table");
    return nullptr;
  }
  std::lock_guard<std::mutex> lock(g_exp_table_mutex);
  if (g_exp_table[dev] || !build) return g_exp_table[dev];
  std::vector<uint16_t> host(65536);
  for (uint32_t i = 0; i < 65536u; i++) host[i] = f32_to_f16_bits(expf(f16_bits_to_f32_host(uint16_t(i))));
  uint16_t* d = nullptr;
  if (hipMalloc((void**)&d, host.size() * 2) != hipSuccess || hipMemcpy(d, host.data(), host.size() * 2, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    if (d) (void)hipFree(d);
    set_error("moe_route: allocating the exponential table failed");
    return nullptr;
  }
  g_exp_table[dev] = d;
  return d;
}

// 0 = done, -1 = error (set_error), 1 = not taken (the caller's per-row path serves the call)
static int mul_mat_id_grouped(const float* dA, const int32_t* dIds, int ids_stride, int id, const ns_expert_group* g, float* dC, int m, int lda,
                              int ldc, int epilogue, const float* dD, int ldd, hipStream_t st) {
  const ns_weight* w0 = g->experts[0];
  const int n_as = int(g->experts.size()), n = w0->n, k = w0->k;
  // fp8 experts: from 65 token rows, while the tiled kernel takes them ("g3_f8", the load's range rule) — every expert of the group
  if (w0->shuf || (k % 64) != 0) return 1;
  if (w0->kind == WK_F8) {
    if (m <= 64) return 1;
    for (const ns_weight* w : g->experts)
      if (!gemm3_takes(w)) return 1;
  }
  const int kpad = k;
  // scratch: ids column + permutation + validity (3 m ints), gathered fp16 rows [m + 1][k], raw products [m + 1][n] (one padding row: a
  // single-row group is launched with two rows — the tiled kernel's minimum — and its second row belongs to the NEXT group, launched later)
  int32_t* ints = static_cast<int32_t*>(stream_scratch(st, size_t(3) * m * 4, SLOT_MOE_IDS));
  _Float16* ag = static_cast<_Float16*>(stream_scratch(st, size_t(m + 1) * kpad * 2, SLOT_MOE_ROWS16));
  float* cg = static_cast<float*>(stream_scratch(st, size_t(m + 1) * n * 4, SLOT_MOE_PRODUCTS));
  if (!ints || !ag || !cg) return 1;
  int32_t *d_col = ints, *d_perm = ints + m, *d_valid = ints + 2 * size_t(m);
  hipLaunchKernelGGL(moe_ids_column_kernel, dim3((m + 255) / 256), dim3(256), 0, st, dIds, ids_stride, id, m, d_col);
  std::vector<int32_t> col(m), perm(m), valid(m);
  if (hipMemcpyAsync(col.data(), d_col, size_t(m) * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    set_error("mul_mat_id: reading the expert ids failed");
    return -1;
  }
  // counting sort by expert; ids outside the group go last (their rows are written as zero products)
  std::vector<int> count(n_as + 1, 0), off(n_as + 2, 0);
  for (int t = 0; t < m; t++) count[col[t] >= 0 && col[t] < n_as ? col[t] : n_as]++;
  for (int e = 0; e <= n_as; e++) off[e + 1] = off[e] + count[e];
  if (w0->kind == WK_F8)  // (the tiled kernel takes fp8 weights from 17 rows: an expert with fewer keeps the call on the per-row kernels)
    for (int e = 0; e < n_as; e++)
      if (count[e] > 0 && count[e] < 17) return 1;
  std::vector<int> fill(off.begin(), off.end() - 1);
  for (int t = 0; t < m; t++) {
    const int e = col[t] >= 0 && col[t] < n_as ? col[t] : n_as;
    perm[fill[e]] = t, valid[fill[e]] = e < n_as ? 1 : 0;
    fill[e]++;
  }
  if (hipMemcpyAsync(d_perm, perm.data(), size_t(m) * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d_valid, valid.data(), size_t(m) * 4, hipMemcpyHostToDevice, st) != hipSuccess) {
    set_error("mul_mat_id: uploading the row order failed");
    return -1;
  }
  {
    const size_t units = size_t(m) * (kpad / 8);
    hipLaunchKernelGGL(moe_gather_rows_kernel, dim3(unsigned((units + 255) / 256)), dim3(256), 0, st, dA, lda, d_perm, m, k, kpad, ag);
    // the padding row: zeros (read by the last group when it has a single row)
    if (hipMemsetAsync(ag + size_t(m) * kpad, 0, size_t(kpad) * 2, st) != hipSuccess) return -1;
  }
  for (int e = 0; e < n_as; e++) {
    const int r = count[e];
    if (!r) continue;
    SmallMArgs a{};
    a.a = nullptr, a.a16 = ag + size_t(off[e]) * kpad, a.lda = kpad, a.m = r < 2 ? 2 : r, a.ldc = n, a.nseg = 1;
    a.seg[0] = {g->experts[e], cg + size_t(off[e]) * n, nullptr};
    a.epilogue = NS_EPI_NONE;
    const hipError_t er = launch_gemm2(a, st);
    if (er == hipErrorNotSupported) {
      // (nothing has been written to dC yet: the per-row path can still serve the whole call)
      (void)hipStreamSynchronize(st);  // the host vectors above are being read by the two uploads
      return 1;
    }
    if (er != hipSuccess) {
      set_error(std::string("mul_mat_id (grouped): ") + hipGetErrorString(er));
      (void)hipStreamSynchronize(st);
      return -1;
    }
  }
  {
    const size_t total = size_t(m) * n;
    hipLaunchKernelGGL(moe_scatter_epilogue_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, st, cg, d_perm, d_valid, m, n, dC, ldc, epilogue, dD, ldd);
  }
  // the uploads read host vectors that die with this frame
  if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) {
    set_error("mul_mat_id (grouped): launch failed");
    return -1;
  }
  return 0;
}
}  // namespace ns
using ns::mul_mat_id_grouped;

extern "C" {

ns_expert_group* ns_hip_expert_group_create(const ns_weight* const* experts, int n_as) {
  if (!experts || n_as <= 0 || n_as > 4096) {
    set_error("expert group: need 1..4096 experts");
    return nullptr;
  }
  const ns_weight* w0 = experts[0];
  std::vector<MoeExpert> host(n_as);
  for (int i = 0; i < n_as; i++) {
    const ns_weight* w = experts[i];
    if (!w || !w0) {
      set_error("expert group: null weight");
      return nullptr;
    }
    // one kernel launch serves every expert: shapes and formats must agree (they do in every MoE checkpoint)
    if (w->n != w0->n || w->k != w0->k || w->kind != w0->kind || w->qtype != w0->qtype || w->blocksize != w0->blocksize ||
        w->scale_dt != w0->scale_dt || w->asym != w0->asym || w->qstride != w0->qstride || w->sstride != w0->sstride ||
        w->zstride != w0->zstride || w->shuf || w->device != w0->device) {
      set_error("expert group: experts differ in shape / format (or carry an activation shuffle)");
      return nullptr;
    }
    host[i] = {reinterpret_cast<const uint8_t*>(w->codes), static_cast<const uint8_t*>(w->scales), w->zps};
  }
  if (w0->kind != WK_INT4 && w0->kind != WK_INT8 && w0->kind != WK_F4 && w0->kind != WK_F8) {
    set_error("expert group: S1..S8, the 4-bit float types and fp8 are supported");
    return nullptr;
  }
  (void)moe_exp_table();  // the router's table, made outside any capture (ns_hip_moe_route); a failure is reported by that entry
  ns_expert_group* g = new ns_expert_group;
  g->experts.assign(experts, experts + n_as);
  if (hipMalloc((void**)&g->table, sizeof(MoeExpert) * n_as) != hipSuccess ||
      hipMemcpy(g->table, host.data(), sizeof(MoeExpert) * n_as, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    set_error("expert group: device table allocation failed");
    if (g->table) (void)hipFree(g->table);
    delete g;
    return nullptr;
  }
  return g;
}

void ns_hip_expert_group_free(ns_expert_group* g) {
  if (!g) return;
  if (g->table) (void)hipFree(g->table);
  delete g;
}

int ns_hip_mul_mat_id(const float* dA, const int32_t* dIds, int ids_stride, int id, const ns_expert_group* g, float* dC,
                      int m, int lda, int ldc, int epilogue, const float* dD, int ldd, void* stream) {
  if (!g || !dA || !dIds || !dC || m <= 0 || id < 0 || id >= ids_stride) {
    set_error("mul_mat_id: bad argument");
    return -1;
  }
  if (m > 65535) {
    set_error("mul_mat_id: at most 65535 token rows per call");
    return -1;
  }
  const ns_weight* w = g->experts[0];
  MoeParams p{};
  p.table = g->table;
  p.n_as = int(g->experts.size());
  p.ids = dIds, p.ids_stride = ids_stride, p.id = id;
  p.qstride = w->qstride, p.sstride = w->sstride, p.zstride = w->zstride;
  p.ksteps = w->ksteps, p.kstep_len = w->kstep_len, p.kind = w->kind;
  p.sps = w->sps, p.srows = w->srows;
  if (!srow_params(w, &p.srow_mul, &p.srow_shift)) {
    set_error("mul_mat_id: group size not expressible for this weight");
    return -1;
  }
  p.scale_dt = w->scale_dt;
  p.asym = w->asym ? 1 : 0;
  p.n = w->n, p.k = w->k, p.m = m;
  p.a = dA, p.lda = lda, p.c = dC, p.ldc = ldc;
  p.epilogue = epilogue, p.d = dD, p.ldd = ldd;
  for (int i = 0; i < 16; i++) p.lut[i] = w->lutf[i];
  p.f8_e5m2 = w->qtype == DT_F8_E5M2 ? 1 : 0;
  const size_t lds = size_t(w->ksteps) * w->kstep_len * 2;
  if (lds > 60 * 1024) {
    set_error("mul_mat_id: K beyond 30720 is not supported by this first version");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  // prefill-sized calls: rows grouped by expert, one tiled GEMM per expert (see moe_gather_rows_kernel)
  static const int grouped_env = getenv("NS_MOE_GROUPED_ROWS") ? atoi(getenv("NS_MOE_GROUPED_ROWS")) : 32;
  const int grouped_set = g_moe_grouped_rows.load();
  const int grouped_from = grouped_set ? grouped_set : grouped_env;
  if (m >= grouped_from && grouped_from > 0) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    (void)hipGetLastError();
    if (!capturing) {
      const int rc = mul_mat_id_grouped(dA, dIds, ids_stride, id, g, dC, m, lda, ldc, epilogue, dD, ldd, st);
      if (rc == 0) g_moe_stats[0]++;
      if (rc <= 0) return rc;  // 0 done, -1 failed; 1: outside the tiled kernel's envelope — the per-row kernels below
      g_moe_stats[3]++;
    }
  }
  // decode-sized calls: one launch of the decode kernel (ns_gemv.hip, XV = 4) per token row — LDS-DMA rings, MFMA on the raw
  // codes, the expert's base pointer picked from the table on the device — instead of this file's VALU loop (Mixtral shapes,
  // one token, 8 x {14336 x 4096, 4096 x 14336} int4: 169 us per MoE FFN layer with the loop, profiles/r04s_moe_mixtral_m1.json)
  static const int gemv_env = getenv("NS_MOE_GEMV_ROWS") ? atoi(getenv("NS_MOE_GEMV_ROWS")) : 8;
  const int gemv_set = g_moe_gemv_rows.load();
  const int moe_gemv_rows = gemv_set ? gemv_set : gemv_env;
  if (m <= moe_gemv_rows && w->single_span && w->kind != WK_F8) {  // (fp8 experts: the loop below)
    bool all = true;
    for (int t = 0; t < m && all; t++) {
      MoeRoute route{g->table, dIds + size_t(t) * ids_stride + id, int(g->experts.size())};
      SmallMArgs a{};
      a.a = dA + size_t(t) * lda, a.lda = lda, a.m = 1, a.ldc = ldc, a.nseg = 1;
      a.seg[0] = {w, dC + size_t(t) * ldc, nullptr};
      a.epilogue = epilogue, a.d = dD ? dD + size_t(t) * ldd : nullptr, a.ldd = ldd;
      a.moe = &route;
      const hipError_t e = launch_gemv(a, st);
      if (e == hipErrorNotSupported && t == 0) {
        all = false;  // outside that kernel's envelope: the loop below serves the whole call
      } else if (e != hipSuccess) {
        set_error(std::string("mul_mat_id launch: ") + hipGetErrorString(e));
        return -1;
      }
    }
    if (all) {
      g_moe_stats[1]++;
      return 0;
    }
  }
  const dim3 grid(w->ntiles, m), block(kMoeThreads);
  if (w->kind == WK_INT8)
    hipLaunchKernelGGL(moe_gemv_kernel<WK_INT8>, grid, block, lds, st, p);
  else if (w->kind == WK_F8)
    hipLaunchKernelGGL(moe_gemv_kernel<WK_F8>, grid, block, lds, st, p);
  else if (w->kind == WK_F4)
    hipLaunchKernelGGL(moe_gemv_kernel<WK_F4>, grid, block, lds, st, p);
  else
    hipLaunchKernelGGL(moe_gemv_kernel<WK_INT4>, grid, block, lds, st, p);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string("mul_mat_id launch: ") + hipGetErrorString(e));
    return -1;
  }
  g_moe_stats[2]++;
  return 0;
}

void ns_hip_moe_stats(uint64_t out[4]) {
  for (int i = 0; i < 4; i++) out[i] = g_moe_stats[i].load();
}

int ns_hip_moe_route(const float* dLogits, int ld_logits, int m, int n_expert, int n_used, int32_t* dIds, int ids_stride, float* dWeights,
                     int w_stride, float* dProbs, void* stream) {
  return ns_hip_moe_route_f(dLogits, ld_logits, m, n_expert, n_used, dIds, ids_stride, dWeights, w_stride, dProbs, 0, stream);
}

int ns_hip_moe_route_f(const float* dLogits, int ld_logits, int m, int n_expert, int n_used, int32_t* dIds, int ids_stride, float* dWeights,
                       int w_stride, float* dProbs, int flags, void* stream) {
  if (!have_device()) return -1;
  if (flags & ~NS_MOE_ROUTE_RAW_WEIGHTS) {
    set_error("moe_route: unknown flag bits (NS_MOE_ROUTE_RAW_WEIGHTS is the only flag)");
    return -1;
  }
  if (n_used < 1 || n_used > 8 || n_expert < n_used || n_expert > 64 || m < 1) {
    set_error("moe_route: need 1 <= n_used <= 8, n_used <= n_expert <= 64 and at least one row");
    return -1;
  }
  if (!dLogits || !dIds || !dWeights || ld_logits < n_expert || ids_stride < n_used || w_stride < n_used) {
    set_error("moe_route: bad argument (null pointer, or a row stride shorter than its row)");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
  (void)hipGetLastError();
  const uint16_t* table = moe_exp_table(!capturing);  // (a synchronous upload: never inside a capture)
  if (!table) {
    if (capturing) set_error("moe_route: the exponential table is not built yet - call ns_hip_warm_up, create an expert group or route once before capturing");
    return -1;
  }
  hipLaunchKernelGGL(moe_route_kernel, dim3(unsigned((m + kRouteWaves - 1) / kRouteWaves)), dim3(kRouteWaves * 64), 0, st, dLogits, ld_logits, m,
                     n_expert, n_used, table, dIds, ids_stride, dWeights, w_stride, dProbs, (flags & NS_MOE_ROUTE_RAW_WEIGHTS) ? 1 : 0);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string("moe_route launch: ") + hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// the entry's name in error texts, by activation
static const char* moe_ffn_name(int act) { return act == NS_EPI_GELU ? "moe_ffn_gelu" : "moe_ffn_silu"; }

// the composition: per selection three ns_hip_mul_mat_id calls (gate with the activation, up with Mul, down) and the weighted sum
static int moe_ffn_composition(const float* dA, int lda, int m, const int32_t* dIds, int ids_stride, const float* dWeights, int w_stride, int n_used,
                               const ns_expert_group* gate, const ns_expert_group* up, const ns_expert_group* down, float* dOut, int ldo,
                               int act, hipStream_t st) {
  const int ff = gate->experts[0]->n, dn = down->experts[0]->n;
  float* t1 = static_cast<float*>(stream_scratch(st, size_t(m) * ff * 4, SLOT_MOE_T1));
  float* t2 = static_cast<float*>(stream_scratch(st, size_t(m) * ff * 4, SLOT_MOE_T2));
  float* t3 = static_cast<float*>(stream_scratch(st, size_t(m) * dn * 4, SLOT_MOE_T3));
  if (!t1 || !t2 || !t3) {
    set_error(std::string(moe_ffn_name(act)) + ": scratch allocation failed");
    return -1;
  }
  for (int i = 0; i < n_used; i++) {
    if (ns_hip_mul_mat_id(dA, dIds, ids_stride, i, gate, t1, m, lda, ff, act, nullptr, 0, st) != 0 ||
        ns_hip_mul_mat_id(dA, dIds, ids_stride, i, up, t2, m, lda, ff, NS_EPI_MUL, t1, ff, st) != 0 ||
        ns_hip_mul_mat_id(t2, dIds, ids_stride, i, down, t3, m, ff, dn, NS_EPI_NONE, nullptr, 0, st) != 0)
      return -1;
    const size_t total = size_t(m) * dn;
    hipLaunchKernelGGL(moe_weighted_add_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, st, dOut, ldo, t3, dn,
                       dWeights ? dWeights + i : nullptr, w_stride, m, dn, i == 0 ? 1 : 0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      set_error(std::string(moe_ffn_name(act)) + " (weighted sum): " + hipGetErrorString(e));
      return -1;
    }
  }
  g_moe_ffn_stats[1]++;
  return 0;
}

// the fused launches: 0 = done, -1 = error, 1 = not taken (nothing written to dOut yet: the composition serves the call)
static int moe_ffn_fused(const float* dA, int lda, int m, const int32_t* dIds, int ids_stride, const float* dWeights, int w_stride, int n_used,
                         const ns_expert_group* gate, const ns_expert_group* up, const ns_expert_group* down, float* dOut, int ldo, int act,
                         hipStream_t st) {
  const ns_weight *wg = gate->experts[0], *wu = up->experts[0], *wd = down->experts[0];
  const int ff = wg->n, n_as = int(gate->experts.size());
  if (wg->kind == WK_F8 || wd->kind == WK_F8 || !wg->single_span || !wu->single_span || !wd->single_span || (ff & 3)) return 1;
  if (int64_t(m) * n_used >= 65536 / std::max(n_used, 1)) return 1;  // (pairs along grid.y, launch_gemv)
  // fp32 intermediate act(gate) * up, [m][n_used][ff]: the down launches round it to fp16 while staging, like every fp32 activation row
  float* inter = static_cast<float*>(stream_scratch(st, size_t(m) * n_used * ff * 4, SLOT_MOE_INTER));
  if (!inter) return 1;
  {
    MoeRoute route{gate->table, dIds, n_as};
    route.table1 = up->table;
    route.pairs = m * n_used, route.nsel = n_used, route.ids_stride = ids_stride;
    route.a_stride = lda, route.c_stride = ff;
    SmallMArgs a{};
    a.a = dA, a.lda = lda, a.m = 1, a.ldc = ff, a.nseg = 2;
    a.seg[0] = {wg, inter, nullptr};
    a.seg[1] = {wu, nullptr, nullptr};
    a.epilogue = act, a.dual = true;  // (GV_DUAL's epilogue picks SiLU or GeLU from this run-time value)
    a.moe = &route;
    const hipError_t e = launch_gemv(a, st);
    if (e == hipErrorNotSupported) return 1;
    if (e != hipSuccess) {
      set_error(std::string(moe_ffn_name(act)) + " (gate / up launch): " + hipGetErrorString(e));
      return -1;
    }
  }
  for (int i = 0; i < n_used; i++) {
    MoeRoute route{down->table, dIds + i, n_as};
    route.pairs = m, route.nsel = 1, route.ids_stride = ids_stride;
    route.w = dWeights ? dWeights + i : nullptr, route.w_stride = w_stride;
    route.a_stride = (long long)n_used * ff, route.c_stride = ldo, route.d_stride = ldo;
    SmallMArgs a{};
    a.a = inter + size_t(i) * ff, a.lda = n_used * ff, a.m = 1, a.ldc = ldo, a.nseg = 1;
    a.seg[0] = {wd, dOut, nullptr};
    a.epilogue = i ? NS_EPI_ADD : NS_EPI_NONE, a.d = i ? dOut : nullptr, a.ldd = ldo;
    a.moe = &route;
    const hipError_t e = launch_gemv(a, st);
    if (e == hipErrorNotSupported && i == 0) {
      g_moe_ffn_stats[2]++;  // (the gate / up launch went out; its result is dropped)
      return 1;
    }
    if (e != hipSuccess) {
      set_error(std::string(moe_ffn_name(act)) + " (down launch): " + hipGetErrorString(e));
      return -1;
    }
  }
  g_moe_ffn_stats[0]++;
  g_moe_ffn_stats[2] += uint64_t(1 + n_used);
  return 0;
}

// the grouped pass (prompt size, never captured): 0 = done, -1 = error, 1 = not taken.  dOut is written by the last launch alone, so whatever is
// refused on the way — a format, a shape, a GEMM launch after others went out — leaves the whole call to the composition.
// One host read-back of the ids; ns_moe_plan.cpp sorts the (row, selection) pairs by expert; one gather into fp16 rows in group order; per
// populated expert, in ascending order (MoePairPlan::launch_rows), one gate / up pair launch of the tiled GEMM — act(gate) * up in registers,
// fp16 out only — and one down launch on that fp16 intermediate; one combine.  Against the composition's n_used x 3 grouped mul_mat_id
// calls: one read-back instead of n_used x 3, groups of n_used x the rows, no fp32 [m][ff] intermediate, no scatter, one weighted sum.
static int moe_ffn_grouped(const float* dA, int lda, int m, const int32_t* dIds, int ids_stride, const float* dWeights, int w_stride, int n_used,
                           const ns_expert_group* gate, const ns_expert_group* up, const ns_expert_group* down, float* dOut, int ldo, int act,
                           hipStream_t st) {
  const ns_weight *wg = gate->experts[0], *wu = up->experts[0], *wd = down->experts[0];
  const int k = wg->k, ff = wg->n, dn = wd->n, n_as = int(gate->experts.size());
  if (wg->kind == WK_F8 || wu->kind == WK_F8 || wd->kind == WK_F8) return 1;  // (fp8 experts: the composition)
  if ((k % 64) != 0 || (ff % 64) != 0) return 1;
  if (wu->kind != wg->kind || wu->qtype != wg->qtype || wu->blocksize != wg->blocksize || wu->scale_dt != wg->scale_dt || wu->asym != wg->asym ||
      wu->qstride != wg->qstride || wu->sstride != wg->sstride || wu->zstride != wg->zstride)
    return 1;  // (a gate / up pair launch needs one format)
  const std::string name = moe_ffn_name(act);
  // the ids, once: rows of ids_stride ints, the last one n_used long
  std::vector<int32_t> ids(size_t(m - 1) * ids_stride + n_used);
  if (hipMemcpyAsync(ids.data(), dIds, ids.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    (void)hipGetLastError();
    set_error(name + " (grouped): reading the expert ids failed");
    return -1;
  }
  MoePairPlan pl;
  if (!moe_pair_plan(ids.data(), ids_stride, m, n_used, n_as, &pl)) return 1;
  const size_t rows = size_t(pl.pairs) + 1, n_pos = size_t(m) * n_used;  // (+ 1: the padding row behind a last group of one row)
  if (rows * size_t(std::max(k, std::max(ff, dn))) >= (size_t(1) << 31)) return 1;
  int32_t* ints = static_cast<int32_t*>(stream_scratch(st, (rows + n_pos) * 4, SLOT_MOE_PAIR_INTS));
  _Float16* ag = static_cast<_Float16*>(stream_scratch(st, rows * k * 2, SLOT_MOE_PAIR_ROWS16));
  _Float16* inter = static_cast<_Float16*>(stream_scratch(st, rows * ff * 2, SLOT_MOE_PAIR_INTER16));
  float* y = static_cast<float*>(stream_scratch(st, rows * dn * 4, SLOT_MOE_PAIR_Y));
  if (!ints || !ag || !inter || !y) return 1;
  int32_t *d_src = ints, *d_pos = ints + rows;
  // one upload of both tables; the stream is idle (the read-back above), so waiting for it here costs the copy alone and the host vectors
  // may die with this frame while the launches below are still running
  std::vector<int32_t> tables(pl.src_row);
  tables.insert(tables.end(), pl.pos.begin(), pl.pos.end());
  if (hipMemcpyAsync(ints, tables.data(), tables.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    (void)hipGetLastError();
    set_error(name + " (grouped): uploading the pair layout failed");
    return -1;
  }
  {
    const size_t units = rows * (k / 8);
    const int vec = (lda & 3) == 0 && (reinterpret_cast<uintptr_t>(dA) & 15) == 0;
    hipLaunchKernelGGL(moe_pair_gather_kernel, dim3(unsigned((units + 255) / 256)), dim3(256), 0, st, dA, lda, d_src, int(rows), k, vec, ag);
  }
  for (int e = 0; e < n_as; e++) {
    const int r = pl.launch_rows[e];
    if (!r) continue;
    const size_t off = size_t(pl.offset[e]);
    SmallMArgs gu{};
    gu.a = nullptr, gu.a16 = ag + off * k, gu.lda = k, gu.m = r, gu.ldc = ff, gu.nseg = 2;
    gu.seg[0] = {gate->experts[e], nullptr, inter + off * ff};
    gu.seg[1] = {up->experts[e], nullptr, nullptr};
    gu.epilogue = act, gu.dual = true, gu.c2 = nullptr;
    SmallMArgs dw{};
    dw.a = nullptr, dw.a16 = inter + off * ff, dw.lda = ff, dw.m = r, dw.ldc = dn, dw.nseg = 1;
    dw.seg[0] = {down->experts[e], y + off * dn, nullptr};
    dw.epilogue = NS_EPI_NONE;
    hipError_t er = launch_gemm2(gu, st);
    if (er == hipSuccess) er = launch_gemm2(dw, st);
    if (er == hipErrorNotSupported) return 1;  // (dOut is untouched)
    if (er != hipSuccess) {
      set_error(name + " (grouped): " + hipGetErrorString(er));
      return -1;
    }
  }
  {
    const size_t units = size_t(m) * ((dn + 3) / 4);
    const int vec_out = (ldo & 3) == 0 && (reinterpret_cast<uintptr_t>(dOut) & 15) == 0;
    hipLaunchKernelGGL(moe_pair_combine_kernel, dim3(unsigned((units + 255) / 256)), dim3(256), 0, st, y, d_pos, dWeights, w_stride, m, n_used, dn,
                       dOut, ldo, vec_out);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(name + " (grouped): " + hipGetErrorString(e));
    return -1;
  }
  g_moe_ffn_stats[3]++;
  return 0;
}

// the block of both activations: by row count the fused decode launches, the grouped pass, else — and wherever those refuse — the composition
static int moe_ffn_block(const float* dA, int lda, int m, const int32_t* dIds, int ids_stride, const float* dWeights, int w_stride, int n_used,
                         const ns_expert_group* gate, const ns_expert_group* up, const ns_expert_group* down, float* dOut, int ldo, int act,
                         void* stream) {
  if (!have_device()) return -1;
  const std::string name = moe_ffn_name(act);
  if (!dA || !dIds || !gate || !up || !down || !dOut || m < 1 || m > 65535 || n_used < 1 || n_used > ids_stride || (dWeights && w_stride < n_used)) {
    set_error(name + ": bad argument");
    return -1;
  }
  const ns_weight *wg = gate->experts[0], *wu = up->experts[0], *wd = down->experts[0];
  if (wu->n != wg->n || wu->k != wg->k || wd->k != wg->n || gate->experts.size() != up->experts.size() || gate->experts.size() != down->experts.size() ||
      lda < wg->k || ldo < wd->n) {
    set_error(name + ": the gate, up and down groups do not form one feed-forward block (shapes, expert counts), or a row stride is too short");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  static const int gemv_env = getenv("NS_MOE_GEMV_ROWS") ? atoi(getenv("NS_MOE_GEMV_ROWS")) : 8;
  const int gemv_set = g_moe_gemv_rows.load();
  const int moe_gemv_rows = gemv_set ? gemv_set : gemv_env;
  if (g_moe_ffn_fused.load() != 0 && m <= moe_gemv_rows) {
    const int rc = moe_ffn_fused(dA, lda, m, dIds, ids_stride, dWeights, w_stride, n_used, gate, up, down, dOut, ldo, act, st);
    if (rc <= 0) return rc;
  }
  // prompt size, outside a capture (the host reads the ids): the grouped pass.  The default threshold is ns_hip_mul_mat_id's grouped one:
  // from there on the composition synchronises with the host as well
  static const int grouped_env = getenv("NS_MOE_GROUPED_ROWS") ? atoi(getenv("NS_MOE_GROUPED_ROWS")) : 32;
  const int grouped_set = g_moe_ffn_grouped_rows.load();
  const int grouped_from = grouped_set ? grouped_set : grouped_env;
  if (grouped_from > 0 && m >= grouped_from) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    (void)hipGetLastError();
    if (!capturing) {
      const int rc = moe_ffn_grouped(dA, lda, m, dIds, ids_stride, dWeights, w_stride, n_used, gate, up, down, dOut, ldo, act, st);
      if (rc <= 0) return rc;
    }
  }
  return moe_ffn_composition(dA, lda, m, dIds, ids_stride, dWeights, w_stride, n_used, gate, up, down, dOut, ldo, act, st);
}

int ns_hip_moe_ffn_silu(const float* dA, int lda, int m, const int32_t* dIds, int ids_stride, const float* dWeights, int w_stride, int n_used,
                        const ns_expert_group* gate, const ns_expert_group* up, const ns_expert_group* down, float* dOut, int ldo, void* stream) {
  return moe_ffn_block(dA, lda, m, dIds, ids_stride, dWeights, w_stride, n_used, gate, up, down, dOut, ldo, NS_EPI_SILU, stream);
}

int ns_hip_moe_ffn_gelu(const float* dA, int lda, int m, const int32_t* dIds, int ids_stride, const float* dWeights, int w_stride, int n_used,
                        const ns_expert_group* gate, const ns_expert_group* up, const ns_expert_group* down, float* dOut, int ldo, void* stream) {
  return moe_ffn_block(dA, lda, m, dIds, ids_stride, dWeights, w_stride, n_used, gate, up, down, dOut, ldo, NS_EPI_GELU, stream);
}

void ns_hip_moe_ffn_stats(uint64_t out[4]) {
  for (int i = 0; i < 4; i++) out[i] = g_moe_ffn_stats[i].load();
}

}  // extern "C"
