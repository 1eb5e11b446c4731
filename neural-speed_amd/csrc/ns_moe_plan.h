// ns_moe_plan.h — the (row, selection) pair layout of the MoE block's grouped pass (ns_moe.hip: ns_hip_moe_ffn_silu / _gelu at prompt size).
// Plain C++: no HIP type, no library header — ns_moe_plan.cpp compiles with any host compiler (tests/tools/moe_plan_main.cpp, tests/test_moe_plan.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ns {

// Pair (t, i) is selection i of token row t, its expert is ids[t * ids_stride + i].  The pairs whose id lies in [0, n_as) are laid out in
// GROUP ORDER: expert 0's pairs first, then expert 1's, ...; inside a group by (t, i) ascending (a stable counting sort).  A gathered
// position j in [0, pairs) is one row of the fp16 activations, of the fp16 intermediate and of the fp32 down products.
struct MoePairPlan {
  int pairs = 0;                     // pairs with an id in range = gathered rows
  std::vector<int32_t> offset;       // [n_as] first gathered position of expert e's group (consecutive: offset[e + 1] = offset[e] + count[e])
  std::vector<int32_t> count;        // [n_as] pairs of expert e (0: no launch for it)
  // [n_as] rows expert e's GEMMs are launched with: count[e], except that a ONE-row group is launched with 2 rows, the tiled kernel's
  // minimum.  Its second row is position offset[e] + 1: the first row of the next populated group — rewritten when that group is launched,
  // which is why the groups go out in ascending expert order — or, for the last group, the padding row at position `pairs`.  Every
  // buffer indexed by position therefore has pairs + 1 rows.
  std::vector<int32_t> launch_rows;
  std::vector<int32_t> src_row;      // [pairs + 1] token row gathered at position j; src_row[pairs] = -1: the padding row (zeros)
  std::vector<int32_t> pos;          // [m * n_used] gathered position of pair t * n_used + i; -1: its id is outside [0, n_as), it is in no group
};

// false (plan untouched): m, n_used or n_as below 1, ids_stride below n_used, or more than 2^30 pairs
bool moe_pair_plan(const int32_t* ids, int ids_stride, int m, int n_used, int n_as, MoePairPlan* plan);

}  // namespace ns
