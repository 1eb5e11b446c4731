// ns_moe_rows.hip — the memory-bound launches around the tiled GEMM's in both grouped forms (ns_hip_mul_mat_id's grouped path, the block
// entries' grouped pass: ns_moe.cpp) and the weighted sum of the block's composition.  Rows are addressed through the pair layout of
// ns_moe_plan.h: src_row (gathered position -> token row) and pos (pair -> gathered position).
#include <hip/hip_runtime.h>

#include "ns_dev.h"
#include "ns_moe.h"

namespace ns {
namespace {
// the id column of a call, contiguous: what ns_hip_mul_mat_id's grouped path reads back (m ints instead of m * ids_stride)
__global__ void moe_ids_column_kernel(const int32_t* __restrict__ ids, int ids_stride, int id, int m, int32_t* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < m) out[t] = ids[size_t(t) * ids_stride + id];
}
// scatter + epilogue of ns_hip_mul_mat_id's grouped path: token row t takes its raw product from gathered position pos[t]
__global__ void moe_scatter_epilogue_kernel(const float* __restrict__ cg, const int32_t* __restrict__ pos, int m, int n, float* __restrict__ c, int ldc,
                                            int epilogue, const float* __restrict__ d, int ldd) {
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gid >= size_t(m) * n) return;
  const int t = int(gid / n), col = int(gid % n);
  const int j = pos[t];
  float v = j >= 0 ? cg[size_t(j) * n + col] : 0.f;  // an id outside the group: a zero product (the per-row kernels do the same)
  const float dv = d ? d[size_t(t) * ldd + col] : 0.f;
  v = epi_apply(v, dv, epilogue);
  c[size_t(t) * ldc + col] = v;
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

bool aligned16(const void* p, int ld) { return (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// one thread per unit, 256 per workgroup
template <class Kern, class... A>
hipError_t launch_units(Kern kern, size_t units, hipStream_t st, A... args) {
  hipLaunchKernelGGL(kern, dim3(unsigned((units + 255) / 256)), dim3(256), 0, st, args...);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_moe_ids_column(const int32_t* ids, int ids_stride, int id, int m, int32_t* out, hipStream_t st) {
  return launch_units(moe_ids_column_kernel, size_t(m), st, ids, ids_stride, id, m, out);
}
hipError_t launch_moe_gather(const float* a, int lda, const int32_t* src_row, int rows, int k, _Float16* out, hipStream_t st) {
  return launch_units(moe_pair_gather_kernel, size_t(rows) * (k / 8), st, a, lda, src_row, rows, k, aligned16(a, lda) ? 1 : 0, out);
}
hipError_t launch_moe_scatter(const float* cg, const int32_t* pos, int m, int n, float* c, int ldc, int epilogue, const float* d, int ldd,
                              hipStream_t st) {
  return launch_units(moe_scatter_epilogue_kernel, size_t(m) * n, st, cg, pos, m, n, c, ldc, epilogue, d, ldd);
}
hipError_t launch_moe_weighted_add(float* out, int ldo, const float* x, int ldx, const float* w, int w_stride, int m, int n, bool first,
                                   hipStream_t st) {
  return launch_units(moe_weighted_add_kernel, size_t(m) * n, st, out, ldo, x, ldx, w, w_stride, m, n, first ? 1 : 0);
}
hipError_t launch_moe_combine(const float* y, const int32_t* pos, const float* w, int w_stride, int m, int n_used, int n, float* out, int ldo,
                              hipStream_t st) {
  return launch_units(moe_pair_combine_kernel, size_t(m) * ((n + 3) / 4), st, y, pos, w, w_stride, m, n_used, n, out, ldo, aligned16(out, ldo) ? 1 : 0);
}

}  // namespace ns
