// Program of tests/test_moe_plan.py: prints the pair layout moe_pair_plan (neural-speed_amd/csrc/ns_moe_plan.cpp) makes of every id table on
// its standard input.  One table per input line:   m n_used n_as ids_stride  id id id ...   (m * ids_stride ids, row-major; the columns
// beyond n_used are padding the plan must not read as ids).  One output line per table:
//   pairs=P offset=.. count=.. launch_rows=.. src_row=.. pos=..      (comma-separated lists)   or   refused
// Plain host C++ (linked with ns_moe_plan.cpp): builds with the library's compiler and with g++, sanitizers included.
#include <cstdio>
#include <vector>

#include "ns_moe_plan.h"

static void print_list(const char* name, const std::vector<int32_t>& v) {
  printf(" %s=", name);
  for (size_t i = 0; i < v.size(); i++) printf(i ? ",%d" : "%d", int(v[i]));
}

int main() {
  int m, n_used, n_as, ids_stride;
  while (scanf("%d %d %d %d", &m, &n_used, &n_as, &ids_stride) == 4) {
    const long long cells = (m > 0 && ids_stride > 0) ? (long long)m * ids_stride : 0;
    if (cells > (1 << 24)) return 2;
    std::vector<int32_t> ids(static_cast<size_t>(cells));
    for (auto& v : ids) {
      int x;
      if (scanf("%d", &x) != 1) return 2;
      v = x;
    }
    // exactly the cells a caller owns: the last row ends behind its n_used ids (a read beyond it is a sanitizer finding)
    size_t owned_cells = ids.size();
    if (cells > 0 && n_used >= 1 && n_used <= ids_stride) owned_cells = static_cast<size_t>(cells - ids_stride + n_used);
    const std::vector<int32_t> owned(ids.begin(), ids.begin() + owned_cells);  // (a fresh allocation of exactly that size)
    ns::MoePairPlan pl;
    if (!ns::moe_pair_plan(owned.empty() ? nullptr : owned.data(), ids_stride, m, n_used, n_as, &pl)) {
      printf("refused\n");
      continue;
    }
    printf("pairs=%d", pl.pairs);
    print_list("offset", pl.offset);
    print_list("count", pl.count);
    print_list("launch_rows", pl.launch_rows);
    print_list("src_row", pl.src_row);
    print_list("pos", pl.pos);
    printf("\n");
  }
  return 0;
}
