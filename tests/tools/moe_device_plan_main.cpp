// Program of tests/test_moe_device_plan.py over neural-speed_amd/csrc/ns_moe_plan.cpp: the decisions and layouts of the block entries'
// device-grouped pass.  One mode per run, one query per input line:
//   plans      gemv_rows grouped_rows ffn_grouped_rows ffn_fused ffn_device_rows  gate_f8 up_f8 down_f8  k ff dn n_as n_used m  single_span shuf
//              all_tiled_f8 gate_up_one_format capturing  gu_kstep dn_kstep i8_mode
//              ->  fused=T,R device=T,R grouped=T,R      (T: tried, R: statically refused)
//   chunks     m n_used n_as ids_stride R  id id id ...   (m * ids_stride ids, row-major; the columns beyond n_used are padding)
//              ->  pairs=P offset=.. count=.. src_row=.. pos=.. chunks=e:first:rows,.. slots=S      or   refused
//   rows       k kstep cap                ->  moe_chunk_rows
//   maxchunks  m n_used n_as R            ->  max=M slots=S : the most chunks moe_chunk_plan makes of ANY table with ids in [-1, n_as)
// Plain host C++ (linked with ns_moe_plan.cpp): builds with the library's compiler and with g++, sanitizers included.
#include <algorithm>
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
  int v[22];
  for (;;) {
    for (int& x : v)
      if (scanf("%d", &x) != 1) return &x == v ? 0 : 2;
    ns::MoeKnobs kn;
    kn.gemv_rows = v[0], kn.grouped_rows = v[1], kn.ffn_grouped_rows = v[2], kn.ffn_fused = v[3], kn.ffn_device_rows = v[4];
    ns::MoeFacts f;
    f.gate_f8 = v[5], f.up_f8 = v[6], f.down_f8 = v[7];
    f.k = v[8], f.ff = v[9], f.dn = v[10], f.n_as = v[11], f.n_used = v[12], f.m = v[13];
    f.single_span = v[14], f.shuf = v[15], f.all_tiled_f8 = v[16], f.gate_up_one_format = v[17], f.capturing = v[18];
    f.gu_kstep = v[19], f.dn_kstep = v[20], f.i8_mode = v[21];
    const ns::MoeFfnPlan p = ns::moe_ffn_plan(kn, f);
    print_candidate("fused", p.fused);
    print_candidate(" device", p.device);
    print_candidate(" grouped", p.grouped);
    printf("\n");
  }
}

static int chunks() {
  int m, n_used, n_as, ids_stride, R;
  while (scanf("%d %d %d %d %d", &m, &n_used, &n_as, &ids_stride, &R) == 5) {
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
    const std::vector<int32_t> owned(ids.begin(), ids.begin() + owned_cells);
    ns::MoeChunkPlan pl;
    if (!ns::moe_chunk_plan(owned.empty() ? nullptr : owned.data(), ids_stride, m, n_used, n_as, R, &pl)) {
      printf("refused\n");
      continue;
    }
    printf("pairs=%d", pl.pairs);
    print_list("offset", pl.offset);
    print_list("count", pl.count);
    print_list("src_row", pl.src_row);
    print_list("pos", pl.pos);
    printf(" chunks=");
    for (size_t i = 0; i < pl.chunks.size(); i++) printf(i ? ",%d:%d:%d" : "%d:%d:%d", int(pl.chunks[i].expert), int(pl.chunks[i].first), int(pl.chunks[i].rows));
    printf(" slots=%d\n", ns::moe_chunk_slots(m, n_used, n_as, R));
  }
  return 0;
}

static int rows() {
  int k, kstep, cap;
  while (scanf("%d %d %d", &k, &kstep, &cap) == 3) printf("%d\n", ns::moe_chunk_rows(k, kstep, cap));
  return 0;
}

static int maxchunks() {
  int m, n_used, n_as, R;
  while (scanf("%d %d %d %d", &m, &n_used, &n_as, &R) == 4) {
    if (m < 1 || n_used < 1 || n_as < 1 || m * n_used > 10 || n_as > 4) return 2;
    const int P = m * n_used;
    std::vector<int32_t> ids(static_cast<size_t>(P), -1);  // an odometer over [-1, n_as) per cell
    size_t most = 0;
    for (;;) {
      ns::MoeChunkPlan pl;
      if (!ns::moe_chunk_plan(ids.data(), n_used, m, n_used, n_as, R, &pl)) return 3;
      most = std::max(most, pl.chunks.size());
      int c = 0;
      while (c < P && ++ids[c] == n_as) ids[c++] = -1;
      if (c == P) break;
    }
    printf("max=%d slots=%d\n", int(most), ns::moe_chunk_slots(m, n_used, n_as, R));
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "plans")) return plans();
  if (argc > 1 && !strcmp(argv[1], "chunks")) return chunks();
  if (argc > 1 && !strcmp(argv[1], "rows")) return rows();
  if (argc > 1 && !strcmp(argv[1], "maxchunks")) return maxchunks();
  return 2;
}
