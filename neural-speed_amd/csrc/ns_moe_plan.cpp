// ns_moe_plan.cpp — which gathered row every (token row, selection) pair of a MoE block call gets: moe_pair_plan, a pure function of the id
// table (no HIP call, no environment, no state).  ns_moe.hip uploads what it says; tests/test_moe_plan.py checks it on the CPU against the
// rule written out independently.
#include "ns_moe_plan.h"

namespace ns {

bool moe_pair_plan(const int32_t* ids, int ids_stride, int m, int n_used, int n_as, MoePairPlan* plan) {
  if (!ids || !plan || m < 1 || n_used < 1 || n_as < 1 || ids_stride < n_used || int64_t(m) * n_used > (int64_t(1) << 30)) return false;
  MoePairPlan& p = *plan;
  const auto in_range = [n_as](int32_t e) { return e >= 0 && e < n_as; };
  p.count.assign(size_t(n_as), 0);
  for (int t = 0; t < m; t++)
    for (int i = 0; i < n_used; i++) {
      const int32_t e = ids[size_t(t) * ids_stride + i];
      if (in_range(e)) p.count[e]++;
    }
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

}  // namespace ns
