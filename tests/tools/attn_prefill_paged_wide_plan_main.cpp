// Program of tests/test_attn_prefill_paged_wide_plan.py: the plan of ns_hip_attn_prefill_paged_wide (attn_prefill_paged_wide_plan,
// neural-speed_amd/csrc/ns_attn_plan.cpp) and a host walk of the request rule its kernel moves K / V tiles by (attn_wide_table_slot, attn_wide_desc,
// attn_wide_k_offset / attn_wide_v_offset, attn_wide_k_lds / attn_wide_v_lds, ns_attn.h).  Three kinds of line:
//   plan   <the call, key=value> | <the fields of the plan>
//   refuse what=<what is wrong> | ok=.. why=..
//   walk   case=.. hs=.. bk=.. kvlen=.. blocks=.. step=.. stepsl=.. stephead=.. ihkv=.. table=<ids> | <one cell per (tile, wave, K / V, request, lane)>
//          cell = pos0:w:kv:u:l:slot:id:base:bytes:offset:lds — slot: the table slot the wave reads, id: what the table holds there, base / bytes: the
//          descriptor (element offset from the pool's base, num_records), offset: the lane's byte offset inside it, lds: where its 16 bytes land
// Host code only: no HIP call is made, no tensor exists — the pointers are made-up addresses.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;

struct Case {
  int hs = 256, cap = 2048, hn = 8, hkv = 8, bs = 2, bk = 16, max_q = 256;
  int head_major = 0, pool_blocks = 0, table_stride = 0;
  long long block_step = 0;
  bool null_table = false, null_qstart = false, null_lens = false;
  unsigned flags = NS_ATTN_FLAG_IS_CAUSAL;
  int k_sl_add = 0;
  float scale = 0.0625f;
  int dst_off = 0, d16 = 0, dst_sl_add = 0;
  bool no_xcd = false;
  int layout = ATTN_FWD_LAYOUT_PLAIN;
  long long step_sl = 0, step_head = 0;  // 0: by the layout
};

static const int g_ints[64] = {0};  // (only its address is used by a plan)

static AttnPrefillWidePlan plan_of(const Case& c, std::string* why) {
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = reinterpret_cast<float*>(uintptr_t(0x10000));
  a.K = reinterpret_cast<decltype(a.K)>(uintptr_t(0x100000));
  a.V = reinterpret_cast<decltype(a.V)>(uintptr_t(0x200000));
  a.dst = reinterpret_cast<float*>(uintptr_t(0x300000 + c.dst_off));
  a.Q_sc = a.K_sc = a.V_sc = a.dst_sc = 1.f;
  a.QK_scale = c.scale;
  a.attn_flags = ns_attn_flags_t(c.flags);
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = c.max_q, a.sl_kv = c.cap;
  a.Q_layout = a.K_layout = a.V_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.dst_layout = ATTN_FWD_LAYOUT(c.layout);
  a.step_q_sl = c.hn * c.hs;
  a.step_dst_sl = c.hn * c.hs + c.dst_sl_add;
  a.step_q_head_num = a.step_dst_head_num = c.hs;
  a.step_q_bs = a.step_dst_bs = a.step_k_bs = a.step_v_bs = 12345;  // (not used)
  a.step_k_head_size = a.step_v_head_size = 1;
  if (c.head_major) {
    a.step_k_sl = a.step_v_sl = c.hs;
    a.step_k_head_num = a.step_v_head_num = (long long)c.bk * c.hs;
  } else {
    a.step_k_sl = a.step_v_sl = (long long)c.hkv * c.hs;
    a.step_k_head_num = a.step_v_head_num = c.hs;
  }
  if (c.step_sl) a.step_k_sl = a.step_v_sl = c.step_sl, a.step_k_head_num = a.step_v_head_num = c.step_head;
  a.step_k_sl += c.k_sl_add;
  AttnPage pg;
  pg.table = c.null_table ? nullptr : g_ints;
  pg.block_shift = attn_block_shift(c.bk);
  pg.table_stride = c.table_stride ? c.table_stride : c.cap / std::max(c.bk, 1);
  pg.pool_blocks = c.pool_blocks ? c.pool_blocks : pg.table_stride * c.bs + 4;
  pg.block_step = c.block_step ? c.block_step : (long long)c.bk * c.hkv * c.hs;
  AttnKnobs kn;
  kn.no_xcd_map = c.no_xcd;
  const void* d16 = c.d16 == 0 ? nullptr : reinterpret_cast<const void*>(uintptr_t(0x400000 + (c.d16 == 2 ? 2 : 0)));
  return attn_prefill_paged_wide_plan(a, d16, kn, pg, c.null_qstart ? nullptr : g_ints, c.null_lens ? nullptr : g_ints + 8, 1, why);
}

static void run_plan(const Case& c) {
  std::string why;
  const AttnPrefillWidePlan pl = plan_of(c, &why);
  const AttnParams& p = pl.pp.a;
  printf("plan bs=%d hn=%d hkv=%d hs=%d maxq=%d cap=%d bk=%d hm=%d dsto=%d d16=%d dstadd=%d noxcd=%d | ok=%d hspad=%d pad=%d grid=%u,%u,%u block=%u lds=%zu nqb=%d "
         "aligned=%d xcd=%d slq=%d slkv=%d kdelta=%d shift=%d bsteps=%lld qstart=%d lens=%d why=%s\n",
         c.bs, c.hn, c.hkv, c.hs, c.max_q, c.cap, c.bk, c.head_major, c.dst_off, c.d16, c.dst_sl_add, int(c.no_xcd), int(pl.ok), p.hs_pad, pl.pad, pl.grid.x,
         pl.grid.y, pl.grid.z, pl.block.x, pl.lds, pl.nqb, pl.aligned, pl.xcd_map, p.sl_q, p.sl_kv, pl.pp.kdelta, pl.pp.pg.block_shift,
         p.step_q_bs + p.step_k_bs + p.step_v_bs + p.step_dst_bs, int(pl.pp.q_start == g_ints), int(pl.pp.kv_lens == g_ints + 8), why.c_str());
}

static void run_refusal(const char* what, const Case& c) {
  std::string why;
  const AttnPrefillWidePlan pl = plan_of(c, &why);
  printf("refuse what=%s | ok=%d why=%s\n", what, int(pl.ok), why.c_str());
}

// every request of every wave of every tile, as attn_wide_paged_kernel's issue() makes it; two kv heads, the walk is kv head ihkv's
static void run_walk(int index, int hs, int bk, int kv_len, int pool_blocks, int head_major, int ihkv, const std::vector<int>& table, long long sl = 0,
                     long long head = 0, long long block_step = 0) {
  AttnPage pg;
  pg.table = table.data(), pg.table_stride = int(table.size()), pg.block_shift = attn_block_shift(bk), pg.pool_blocks = pool_blocks;
  const long long step_sl = sl ? sl : (head_major ? hs : 2 * hs), step_head = sl ? head : (head_major ? (long long)bk * hs : hs);
  pg.block_step = block_step ? block_step : (long long)bk * 2 * hs;
  printf("walk case=%d hs=%d bk=%d kvlen=%d blocks=%d step=%lld stepsl=%lld stephead=%lld ihkv=%d table=", index, hs, bk, kv_len, pool_blocks, pg.block_step,
         step_sl, step_head, ihkv);
  for (size_t i = 0; i < table.size(); i++) printf("%s%d", i ? "," : "", table[i]);
  printf(" |");
  for (int pos0 = 0; pos0 < kv_len; pos0 += kA2KB)
    for (int w = 0; w < 4; w++) {
      const int slot = attn_wide_table_slot(pg, pos0, w, kv_len);
      const AttnWideDesc d = attn_wide_desc(pg, table[slot], pos0, w, kv_len, ihkv, step_sl, step_head, hs);
      for (int kv = 0; kv < 2; kv++)
        for (int u = 0; u < kAwReq; u++)
          for (int l = 0; l < 64; l++)
            printf(" %d:%d:%d:%d:%d:%d:%d:%lld:%u:%u:%d", pos0, w, kv, u, l, slot, table[slot], d.base, d.bytes,
                   kv ? attn_wide_v_offset(u, l, step_sl, hs) : attn_wide_k_offset(u, l, step_sl, hs), (kv ? attn_wide_v_lds(w, u) : attn_wide_k_lds(w, u)) + 16 * l);
    }
  printf("\n");
}

// the pools of the far-address tests, whose numbers (tests/tools/attn_far_layout.py) the caller passes:
//   far  hs bk cap requests max_q pool_blocks block_step step_sl step_head   -> far <the call> | ok=.. pad=.. why=..
//   walk hs bk kv_len pool_blocks block_step step_sl step_head ihkv id id ..   -> one walk line (case -1)
static int from_arguments(int argc, char** argv) {
  const auto at = [&](int i) { return atoll(argv[i]); };
  if (std::string(argv[1]) == "far" && argc == 11) {
    Case c;
    c.hn = 4, c.hkv = 2, c.hs = int(at(2)), c.bk = int(at(3)), c.cap = int(at(4)), c.bs = int(at(5)), c.max_q = int(at(6)), c.pool_blocks = int(at(7));
    c.block_step = at(8), c.step_sl = at(9), c.step_head = at(10);
    std::string why;
    const AttnPrefillWidePlan pl = plan_of(c, &why);
    printf("far hs=%d bk=%d blocks=%d step=%lld stepsl=%lld stephead=%lld | ok=%d pad=%d why=%s\n", c.hs, c.bk, c.pool_blocks, c.block_step, c.step_sl, c.step_head,
           int(pl.ok), pl.pad, why.c_str());
    return 0;
  }
  if (std::string(argv[1]) == "walk" && argc > 10) {
    std::vector<int> table;
    for (int i = 10; i < argc; i++) table.push_back(int(at(i)));
    run_walk(-1, int(at(2)), int(at(3)), int(at(4)), int(at(5)), 0, int(at(9)), table, at(7), at(8), at(6));
    return 0;
  }
  fprintf(stderr, "usage: far .. | walk ..\n");
  return 2;
}

int main(int argc, char** argv) {
  if (argc > 1) return from_arguments(argc, argv);
  const int groups[][2] = {{8, 8}, {8, 1}, {16, 16}};
  int n = 0;
  for (int bk : {16, 64, 256})
    for (int bs : {1, 3, 8})
      for (const auto& g : groups)
        for (int hs : {136, 160, 192, 248, 256})
          for (int max_q : {1, 127, 128, 129, 2048})
            for (int cap : {200, 2048}) {
              Case c;
              c.bs = bs, c.hn = g[0], c.hkv = g[1], c.hs = hs, c.bk = bk, c.max_q = max_q, c.cap = (cap + bk - 1) / bk * bk;
              c.head_major = n & 1, c.dst_off = (n / 3) % 4 == 3 ? 4 : 0, c.d16 = (n / 5) % 3, c.dst_sl_add = (n / 7) % 5 == 4 ? 2 : 0, c.no_xcd = (n / 11) % 4 == 3;
              n++;
              run_plan(c);
            }
  Case c;
  run_refusal("none", c);
  c = Case(), c.null_qstart = true; run_refusal("null_qstart", c);
  c = Case(), c.null_lens = true; run_refusal("null_lens", c);
  c = Case(), c.layout = ATTN_FWD_LAYOUT_NTILE48_ROWPACK4; run_refusal("layout", c);
  c = Case(), c.bs = 0; run_refusal("no_requests", c);
  c = Case(), c.hs = 140; run_refusal("head_size_140", c);
  c = Case(), c.hs = 264; run_refusal("head_size_264", c);
  c = Case(), c.hs = 128; run_refusal("head_size_128", c);
  c = Case(), c.hs = 64; run_refusal("head_size_64", c);
  c = Case(), c.hn = 8, c.hkv = 3; run_refusal("head_group", c);
  c = Case(), c.max_q = 0; run_refusal("max_q_0", c);
  c = Case(), c.cap = 0, c.table_stride = 1; run_refusal("capacity_0", c);
  c = Case(), c.bk = 48, c.table_stride = 2048 / 48; run_refusal("block_keys_48", c);
  c = Case(), c.bk = 512, c.table_stride = 4; run_refusal("block_keys_512", c);
  c = Case(), c.table_stride = 2048 / 16 - 1; run_refusal("capacity", c);
  c = Case(), c.null_table = true; run_refusal("null_table", c);
  c = Case(), c.pool_blocks = -1; run_refusal("pool_blocks", c);
  c = Case(), c.block_step = 16 * 8 * 256 - 8; run_refusal("block_step_small", c);
  c = Case(), c.k_sl_add = 4, c.block_step = 2 * 16 * 8 * 256; run_refusal("kv_rows_unaligned", c);
  c = Case(), c.hn = 65536, c.hkv = 65536, c.bs = 2048, c.max_q = 2048, c.block_step = 16ll * 65536 * 256; run_refusal("grid_limit", c);  // 16 * 65536 * 2048 = 2^31 workgroups
  c = Case(), c.hn = 32768, c.hkv = 32768, c.bs = 2048, c.max_q = 2048, c.block_step = 16ll * 32768 * 256; run_refusal("grid_limit_below", c);
  c = Case(), c.flags |= NS_ATTN_FLAG_IS_ALIBI8; run_refusal("alibi", c);
  c = Case(), c.flags |= NS_ATTN_FLAG_IS_TANH30; run_refusal("tanh", c);
  c = Case(), c.scale = 0.f; run_refusal("scale_0", c);
  c = Case(), c.scale = -0.0625f; run_refusal("scale_negative", c);
  c = Case(), c.scale = 1.f / 0.f; run_refusal("scale_inf", c);
  c = Case(), c.bk = 256, c.table_stride = 8, c.hn = c.hkv = 16512, c.block_step = 256ll * 16512 * 256; run_refusal("descriptor_span", c);  // 255 rows of 16512 * 256 halves: above 2 GiB
  c = Case(), c.bk = 256, c.table_stride = 8, c.hn = c.hkv = 16512, c.block_step = 256ll * 16512 * 256, c.head_major = 1; run_refusal("descriptor_span_head_major", c);  // head-major: 255 rows of 256 halves

  // the walk: live blocks in a permutation, junk behind them, bad ids inside the live length
  run_walk(0, 256, 16, 130, 40, 0, 1, {7, 3, 39, 0, 12, 5, 9, 1, 2, -1, 40, 1 << 30, -5, 17, 4, 4});  // three tiles, the last of two keys
  run_walk(1, 256, 64, 65, 6, 1, 0, {4, 2, 6, -1});                                                   // head-major, a tile of one key
  run_walk(2, 160, 256, 300, 3, 0, 0, {1, 0, 99, -1});                                                // padded, a page holds four tiles
  run_walk(3, 136, 32, 64, 9, 1, 1, {8, 0, -1, 9, 123456});                                           // padded, head-major, ends on a tile
  run_walk(4, 248, 16, 100, 8, 0, 1, {3, 8, -1, 2, 0, 5, 6, 44, 45});                                 // bad ids INSIDE the live length
  return 0;
}
