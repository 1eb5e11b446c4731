// ns_moe.h — what the files of the mixture-of-experts family share: the expert table's row, the group, the loop kernel's arguments and the
// launch_moe_* wrappers, each owning its kernel's grid arithmetic.  Which file holds what: docs/kernels/other.md, "MoE: files and paths".
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "ns_common.h"

namespace ns {

// one row of an expert group's device table: what the decode kernel (ns_gemv.hip, XV = 4) and the loop kernel look up by expert id
struct MoeExpertRow {
  const uint8_t* codes;
  const uint8_t* scales;
  const int8_t* zps;
};

// a call of the loop kernel: one workgroup per (column tile, token row), the row's expert read from ids on the device
struct MoeParams {
  const MoeExpertRow* table;
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

inline int moe_fail(const std::string& msg) { return set_error(msg), -1; }
bool stream_is_capturing(hipStream_t st);  // ns_moe.cpp; a failed query counts as yes, the thread's last-error slot is left clean
// ns_moe_loop.hip: moe_gemv_kernel<p.kind> over (ntiles, p.m) workgroups, the staged row (ksteps * kstep_len fp16) in dynamic LDS
hipError_t launch_moe_loop(const MoeParams& p, int ntiles, hipStream_t st);
// ns_moe_rows.hip — ids_column: out[t] = ids[t * ids_stride + id].  gather: fp32 rows a[src_row[j]] -> fp16 out[j][k], j < rows (src_row < 0:
// zeros; k a multiple of 8).  scatter: c[t] = epi(pos[t] >= 0 ? cg[pos[t]] : 0, d[t]), t < m.  weighted_add: out = (first ? 0 : out) +
// w[t * w_stride] * x (w == nullptr: 1).  combine: out[t] = sum_i w[t][i] * y[pos[t * n_used + i]] over the selections with pos >= 0
hipError_t launch_moe_ids_column(const int32_t* ids, int ids_stride, int id, int m, int32_t* out, hipStream_t st);
hipError_t launch_moe_gather(const float* a, int lda, const int32_t* src_row, int rows, int k, _Float16* out, hipStream_t st);
hipError_t launch_moe_scatter(const float* cg, const int32_t* pos, int m, int n, float* c, int ldc, int epilogue, const float* d, int ldd,
                              hipStream_t st);
hipError_t launch_moe_weighted_add(float* out, int ldo, const float* x, int ldx, const float* w, int w_stride, int m, int n, bool first,
                                   hipStream_t st);
hipError_t launch_moe_combine(const float* y, const int32_t* pos, const float* w, int w_stride, int m, int n_used, int n, float* out, int ldo,
                              hipStream_t st);
// ns_moe_group.hip — moe_pair_sort_kernel, one workgroup: the pair layout of moe_chunk_plan (ns_moe_plan.h) and its chunk lists for two chunk
// sizes, from the ids on the device.  src_row, pos: [pairs]; a chunk list: its count, then {expert, first position, rows} x slots
struct MoeDevSort {
  const int32_t* ids;
  int ids_stride, n_used, pairs, n_as;  // pairs = m * n_used <= kMoeDevMaxPairs
  int r_gu, r_dn, slots_gu, slots_dn;   // rows per chunk and the host's bound of the chunk count (moe_chunk_slots), per list
  int32_t *src_row, *pos, *chunks_gu, *chunks_dn;
};
hipError_t launch_moe_pair_sort(const MoeDevSort& a, hipStream_t st);

}  // namespace ns

struct ns_expert_group {
  std::vector<const ns_weight*> experts;
  ns::MoeExpertRow* table = nullptr;  // device
};
