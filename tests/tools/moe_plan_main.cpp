// Program of tests/test_moe_plan.py, two modes over neural-speed_amd/csrc/ns_moe_plan.cpp.
// Without arguments (or with `min_group_rows N`): prints the pair layout moe_pair_plan makes of every id table on its standard input.  One
// table per input line:   m n_used n_as ids_stride  id id id ...   (m * ids_stride ids, row-major; the columns beyond n_used are padding
// the plan must not read as ids).  One output line per table:
//   pairs=P offset=.. count=.. launch_rows=.. src_row=.. pos=..      (comma-separated lists)   or   refused
// With `plans`: one decision per input line,
//   mm|ffn  gemv_rows grouped_rows ffn_grouped_rows ffn_fused  gate_f8 up_f8 down_f8  k ff dn n_as n_used m  single_span shuf all_tiled_f8
//           gate_up_one_format capturing
// answered by   grouped=T,R decode=T,R min_group_rows=N   or   fused=T,R grouped=T,R   (T: tried, R: statically refused), and
//   fit m n_used   /   addressable rows k ff dn   by the predicate's 0 or 1.
// Plain host C++ (linked with ns_moe_plan.cpp): builds with the library's compiler and with g++, sanitizers included.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ns_moe_plan.h"

static void print_list(const char* name, const std::vector<int32_t>& v) {
  printf(" %s=", name);
  for (size_t i = 0; i < v.size(); i++) printf(i ? ",%d" : "%d", int(v[i]));
}

static void print_candidate(const char* name, const ns::MoeCandidate& c) { printf("%s=%d,%d", name, c.tried ? 1 : 0, c.refused ? 1 : 0); }

static int plans() {
  char what[16];
  while (scanf("%15s", what) == 1) {
    if (!strcmp(what, "fit") || !strcmp(what, "addressable")) {
      long long v[4] = {0, 0, 0, 0};
      const int want = what[0] == 'f' ? 2 : 4;
      for (int i = 0; i < want; i++)
        if (scanf("%lld", &v[i]) != 1) return 2;
      printf("%d\n", what[0] == 'f' ? int(ns::moe_pairs_fit_grid(int(v[0]), int(v[1])))
                                    : int(ns::moe_rows_addressable(size_t(v[0]), int(v[1]), int(v[2]), int(v[3]))));
      continue;
    }
    int v[18];
    for (int& x : v)
      if (scanf("%d", &x) != 1) return 2;
    ns::MoeKnobs kn;
    kn.gemv_rows = v[0], kn.grouped_rows = v[1], kn.ffn_grouped_rows = v[2], kn.ffn_fused = v[3];
    ns::MoeFacts f;
    f.gate_f8 = v[4], f.up_f8 = v[5], f.down_f8 = v[6];
    f.k = v[7], f.ff = v[8], f.dn = v[9], f.n_as = v[10], f.n_used = v[11], f.m = v[12];
    f.single_span = v[13], f.shuf = v[14], f.all_tiled_f8 = v[15], f.gate_up_one_format = v[16], f.capturing = v[17];
    if (!strcmp(what, "mm")) {
      const ns::MoeMmPlan p = ns::moe_mm_plan(kn, f);
      print_candidate("grouped", p.grouped);
      print_candidate(" decode", p.decode);
      printf(" min_group_rows=%d\n", p.min_group_rows);
    } else {
      const ns::MoeFfnPlan p = ns::moe_ffn_plan(kn, f);
      print_candidate("fused", p.fused);
      print_candidate(" grouped", p.grouped);
      printf("\n");
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "plans")) return plans();
  const int min_group_rows = argc > 2 && !strcmp(argv[1], "min_group_rows") ? atoi(argv[2]) : 0;
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
    if (!ns::moe_pair_plan(owned.empty() ? nullptr : owned.data(), ids_stride, m, n_used, n_as, &pl, min_group_rows)) {
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
