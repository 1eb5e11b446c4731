// ns_moe_plan.cpp — the decisions of ns_moe_plan.h as pure functions (no HIP call, no environment, no state); tests/test_moe_plan.py checks
// them on the CPU against the rules written out independently.
#include "ns_moe_plan.h"

#include <algorithm>

namespace ns {

MoeMmPlan moe_mm_plan(const MoeKnobs& kn, const MoeFacts& f) {
  MoeMmPlan p;
  p.grouped.tried = kn.grouped_rows > 0 && f.m >= kn.grouped_rows && !f.capturing;  // (the host reads the ids)
  // no activation shuffle, K in 64s; fp8: the tiled kernel takes it from 65 rows, and only experts inside its range rule
  p.grouped.refused = f.shuf || f.k % 64 || (f.gate_f8 && (f.m <= 64 || !f.all_tiled_f8));
  p.min_group_rows = f.gate_f8 ? 17 : 0;
  p.decode.tried = f.m <= kn.gemv_rows;
  p.decode.refused = !f.single_span || f.gate_f8;
  return p;
}

MoeFfnPlan moe_ffn_plan(const MoeKnobs& kn, const MoeFacts& f) {
  MoeFfnPlan p;
  p.fused.tried = kn.ffn_fused != 0 && f.m <= kn.gemv_rows;
  // (ff & 3: the rows of the fp32 intermediate must stay 16-byte aligned; an fp8 up group is left to launch_gemv's one-format rule)
  p.fused.refused = f.gate_f8 || f.down_f8 || !f.single_span || (f.ff & 3) || !moe_pairs_fit_grid(f.m, f.n_used);
  // the device-grouped pass reads nothing on the host: capturing or not.  Its launches stage several fp16 rows (whole k-steps of both K,
  // as plan_activations of ns_gemv_plan.cpp asks), look the expert up in the decode kernel's addressing and sort the pairs in one workgroup
  p.device.tried = kn.ffn_device_rows > 0 && f.m <= kn.ffn_device_rows;
  p.device.refused = f.gate_f8 || f.up_f8 || f.down_f8 || !f.single_span || !f.gate_up_one_format || f.gu_kstep <= 0 || f.dn_kstep <= 0 ||
                     (f.gu_kstep > 0 && f.k % f.gu_kstep) || (f.dn_kstep > 0 && f.ff % f.dn_kstep) ||
                     int64_t(f.m) * f.n_used > kMoeDevMaxPairs || f.i8_mode;
  p.grouped.tried = kn.ffn_grouped_rows > 0 && f.m >= kn.ffn_grouped_rows && !f.capturing;
  // (a gate / up pair launch needs one format)
  p.grouped.refused = f.gate_f8 || f.up_f8 || f.down_f8 || f.k % 64 || f.ff % 64 || !f.gate_up_one_format;
  return p;
}

bool moe_pairs_fit_grid(int m, int n_used) { return int64_t(m) * n_used < 65536 / std::max(n_used, 1); }
bool moe_rows_addressable(size_t rows, int k, int ff, int dn) { return rows * size_t(std::max(k, std::max(ff, dn))) < (size_t(1) << 31); }

bool moe_pair_plan(const int32_t* ids, int ids_stride, int m, int n_used, int n_as, MoePairPlan* plan, int min_group_rows) {
  if (!ids || !plan || m < 1 || n_used < 1 || n_as < 1 || ids_stride < n_used || int64_t(m) * n_used > (int64_t(1) << 30)) return false;
  const auto in_range = [n_as](int32_t e) { return e >= 0 && e < n_as; };
  std::vector<int32_t> count(size_t(n_as), 0);
  for (int t = 0; t < m; t++)
    for (int i = 0; i < n_used; i++) {
      const int32_t e = ids[size_t(t) * ids_stride + i];
      if (in_range(e)) count[e]++;
    }
  for (int e = 0; e < n_as; e++)
    if (count[e] > 0 && count[e] < min_group_rows) return false;
  MoePairPlan& p = *plan;
  p.count.swap(count);
  p.offset.assign(size_t(n_as), 0);
  p.launch_rows.assign(size_t(n_as), 0);
  int32_t at = 0;
  for (int e = 0; e < n_as; e++) {
    p.offset[e] = at;
    p.launch_rows[e] = p.count[e] == 1 ? 2 : p.count[e];
    at += p.count[e];
  }
  p.pairs = at;
  p.src_row.assign(size_t(at) + 1, -1);
  p.pos.assign(size_t(m) * n_used, -1);
  std::vector<int32_t> fill(p.offset);
  for (int t = 0; t < m; t++)  // (row, selection) ascending: stable inside every group
    for (int i = 0; i < n_used; i++) {
      const int32_t e = ids[size_t(t) * ids_stride + i];
      if (!in_range(e)) continue;
      const int32_t j = fill[e]++;
      p.src_row[j] = t;
      p.pos[size_t(t) * n_used + i] = j;
    }
  return true;
}

int moe_chunk_rows(int k, int kstep, int cap) {
  if (k < 1 || kstep < 1) return 1;
  const int64_t ks = (int64_t(k) + kstep - 1) / kstep;
  const int64_t fit = int64_t(kMoeChunkALds) / ((ks * kstep + 8) * 2);
  int64_t r = std::min<int64_t>(kMoeChunkMaxRows, fit);
  if (cap > 0) r = std::min<int64_t>(r, cap);
  return int(std::max<int64_t>(r, 1));
}

bool moe_chunk_plan(const int32_t* ids, int ids_stride, int m, int n_used, int n_as, int R, MoeChunkPlan* out) {
  MoePairPlan pp;
  if (!out || R < 1 || R > kMoeChunkMaxRows || !moe_pair_plan(ids, ids_stride, m, n_used, n_as, &pp)) return false;
  MoeChunkPlan& p = *out;
  p.pairs = pp.pairs;
  p.offset.swap(pp.offset);
  p.count.swap(pp.count);
  p.pos.swap(pp.pos);
  p.src_row.assign(size_t(m) * n_used, -1);
  std::copy(pp.src_row.begin(), pp.src_row.begin() + pp.pairs, p.src_row.begin());
  p.chunks.clear();
  for (int e = 0; e < n_as; e++)
    for (int32_t c = 0; c * R < p.count[e]; c++) p.chunks.push_back({e, p.offset[e] + c * R, std::min<int32_t>(R, p.count[e] - c * R)});
  return true;
}

int moe_chunk_slots(int m, int n_used, int n_as, int R) {
  if (m < 1 || n_used < 1 || n_as < 1 || R < 1) return 0;
  const int64_t pairs = int64_t(m) * n_used;
  return int((pairs + std::min<int64_t>(n_as, pairs) * (R - 1)) / R);
}

}  // namespace ns
