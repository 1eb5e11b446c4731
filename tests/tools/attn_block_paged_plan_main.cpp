// Program of tests/test_attn_block_paged_plan.py: the plan of ns_hip_attn_block_paged (attn_block_paged_plan, neural-speed_amd/csrc/ns_attn_plan.cpp), the
// workspace size function's value and the live rule the range workgroups and the merge run (attn_block_live, ns_attn.h).  Three kinds of line:
//   plan   <the call, key=value> | <the fields of the plan>
//   refuse what=<what is wrong> | ok=.. why=..
//   live   plan=<index> dyn=<0 / 1> nsplit=.. kps=.. cap=.. | <kps:live of every live length 0 .. cap, blank-separated>
// Host code only: no HIP call is made, no tensor exists — the pointers are made-up addresses.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;

struct Case {
  int hs = 128, cap = 2048, hn = 8, hkv = 8, bs = 2, bk = 16, max_q = 16;
  int head_major = 0;
  int pool_blocks = 0;       // 0: one block per table entry and four spare
  long long block_step = 0;  // 0: a block's own size
  int table_stride = 0;      // 0: cap / bk
  bool null_table = false, null_qstart = false, null_lens = false;
  unsigned flags = NS_ATTN_FLAG_IS_CAUSAL;
  int k_sl_add = 0;  // added to K's row stride
  bool dyn = true;
};

static const int g_ints[64] = {0};  // (only its address is used by a plan)

static AttnBlockPagedPlan plan_of(const Case& c, std::string* why) {
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = reinterpret_cast<float*>(uintptr_t(0x10000));
  a.K = reinterpret_cast<decltype(a.K)>(uintptr_t(0x100000));
  a.V = reinterpret_cast<decltype(a.V)>(uintptr_t(0x200000));
  a.dst = reinterpret_cast<float*>(uintptr_t(0x300000));
  a.Q_sc = a.K_sc = a.V_sc = a.dst_sc = 1.f;
  a.QK_scale = 0.125f;
  a.attn_flags = ns_attn_flags_t(c.flags);
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = c.max_q, a.sl_kv = c.cap;
  a.Q_layout = a.K_layout = a.V_layout = a.dst_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.step_q_sl = a.step_dst_sl = c.hn * c.hs;
  a.step_q_head_num = a.step_dst_head_num = c.hs;
  a.step_k_head_size = a.step_v_head_size = 1;
  if (c.head_major) {
    a.step_k_sl = a.step_v_sl = c.hs;
    a.step_k_head_num = a.step_v_head_num = (long long)c.bk * c.hs;
  } else {
    a.step_k_sl = a.step_v_sl = c.hkv * c.hs;
    a.step_k_head_num = a.step_v_head_num = c.hs;
  }
  a.step_k_sl += c.k_sl_add;
  AttnPage pg;
  pg.table = c.null_table ? nullptr : g_ints;
  pg.block_shift = attn_block_shift(c.bk);
  pg.table_stride = c.table_stride ? c.table_stride : c.cap / std::max(c.bk, 1);
  pg.pool_blocks = c.pool_blocks ? c.pool_blocks : pg.table_stride * c.bs + 4;
  pg.block_step = c.block_step ? c.block_step : (long long)c.bk * c.hkv * c.hs;
  AttnKnobs kn;
  kn.dyn_ranges = c.dyn;
  return attn_block_paged_plan(a, nullptr, kn, pg, c.null_qstart ? nullptr : g_ints, c.null_lens ? nullptr : g_ints, 1, why);
}

static void run_plan(const Case& c) {
  std::string why;
  const AttnBlockPagedPlan pl = plan_of(c, &why);
  const AttnSplitParams& sp = pl.pp.sp;
  printf("plan bs=%d hn=%d hkv=%d hs=%d maxq=%d cap=%d bk=%d hm=%d | ok=%d hspad=%d grid=%u,%u,%u block=%u mgrid=%u,%u,%u nsplit=%d kps=%d gfull=%d dyn=%d "
         "pbytes=%zu ws=%zu slq=%d slkv=%d kdelta=%d shift=%d why=%s\n",
         c.bs, c.hn, c.hkv, c.hs, c.max_q, c.cap, c.bk, c.head_major, int(pl.ok), pl.hs_pad, pl.grid.x, pl.grid.y, pl.grid.z, pl.block.x, pl.merge_grid.x,
         pl.merge_grid.y, pl.merge_grid.z, sp.nsplit, sp.keys_per_split, sp.g_full, sp.dyn_min_keys, pl.partial_bytes,
         attn_block_paged_ws_bytes(AttnKnobs(), c.bs, c.hn, c.hkv, c.hs, c.max_q, c.cap), sp.a.sl_q, sp.a.sl_kv, sp.kdelta, pl.pp.pg.block_shift, why.c_str());
}

static void run_refusal(const char* what, const Case& c) {
  std::string why;
  const AttnBlockPagedPlan pl = plan_of(c, &why);
  printf("refuse what=%s | ok=%d why=%s\n", what, int(pl.ok), why.c_str());
}

static void run_live(int index, Case c, bool dyn) {
  c.dyn = dyn;
  std::string why;
  const AttnBlockPagedPlan pl = plan_of(c, &why);
  const AttnSplitParams& sp = pl.pp.sp;
  printf("live plan=%d dyn=%d nsplit=%d kps=%d cap=%d minkeys=%d |", index, int(dyn), sp.nsplit, sp.keys_per_split, c.cap, sp.dyn_min_keys);
  for (int n = 0; n <= c.cap; n++) {
    const AttnBlockLive lv = attn_block_live(n, sp.nsplit, sp.keys_per_split, sp.dyn_min_keys);
    printf(" %d:%d", lv.kps, lv.live);
  }
  printf("\n");
}

int main() {
  const int groups[][2] = {{8, 8}, {8, 2}, {8, 1}, {71, 1}};  // (heads, kv heads): the head layouts of tests/test_attn_rows_plan.py
  int n = 0;
  for (int bk : {16, 32, 128, 256})
    for (int bs : {1, 2, 8, 33})
      for (const auto& g : groups)
        for (int hs : {64, 128})
          for (int max_q : {1, 2, 16, 17, 64, 127, 300})
            for (int cap : {1, 255, 256, 300, 2048, 8192}) {
              Case c;
              c.bs = bs, c.hn = g[0], c.hkv = g[1], c.hs = hs, c.bk = bk, c.max_q = max_q, c.cap = (cap + bk - 1) / bk * bk, c.head_major = n++ & 1;
              run_plan(c);
            }
  Case c;
  run_refusal("none", c);
  c = Case(), c.null_qstart = true;
  run_refusal("null_qstart", c);
  c = Case(), c.null_lens = true;
  run_refusal("null_lens", c);
  c = Case(), c.hs = 80;
  run_refusal("head_size_80", c);
  c = Case(), c.hs = 256;
  run_refusal("head_size_256", c);
  c = Case(), c.flags |= NS_ATTN_FLAG_IS_ALIBI8;
  run_refusal("alibi", c);
  c = Case(), c.flags |= NS_ATTN_FLAG_IS_TANH30;
  run_refusal("tanh", c);
  c = Case(), c.max_q = 0;
  run_refusal("max_q_0", c);
  c = Case(), c.hn = 4096, c.hkv = 1, c.max_q = 1024;  // 4096 * 1024 / 64 = 65536 slot blocks
  run_refusal("grid_limit", c);
  c = Case(), c.hn = 4096, c.hkv = 1, c.max_q = 1023;  // 65472: served
  run_refusal("grid_limit_below", c);
  c = Case(), c.hn = 8, c.hkv = 3;
  run_refusal("head_group", c);
  c = Case(), c.bk = 48, c.table_stride = 2048 / 48;
  run_refusal("block_keys_48", c);
  c = Case(), c.bk = 8, c.table_stride = 256;
  run_refusal("block_keys_8", c);
  c = Case(), c.bk = 512, c.table_stride = 4;
  run_refusal("block_keys_512", c);
  c = Case(), c.table_stride = 2048 / 16 - 1;
  run_refusal("capacity", c);
  c = Case(), c.null_table = true;
  run_refusal("null_table", c);
  c = Case(), c.pool_blocks = -1;
  run_refusal("pool_blocks", c);
  c = Case(), c.block_step = 16 * 8 * 128 - 8;
  run_refusal("block_step_small", c);
  c = Case(), c.block_step = 16 * 8 * 128 + 4;
  run_refusal("block_step_unaligned", c);
  c = Case(), c.k_sl_add = 4, c.block_step = 2 * 16 * 8 * 128;
  run_refusal("kv_rows_unaligned", c);
  // the live rule over every live length of a few plans, with the dynamic ranges on and off
  const int live_cases[][5] = {{1, 8, 8, 16, 512}, {2, 8, 2, 2, 2048}, {8, 8, 1, 1, 4096}, {33, 8, 8, 64, 1024}, {1, 8, 2, 127, 300 / 4 * 4 + 4}, {1, 8, 8, 4, 64}};
  for (int i = 0; i < 6; i++)
    for (int dyn = 0; dyn < 2; dyn++) {
      Case lc;
      lc.bs = live_cases[i][0], lc.hn = live_cases[i][1], lc.hkv = live_cases[i][2], lc.max_q = live_cases[i][3], lc.cap = live_cases[i][4];
      lc.cap = (lc.cap + lc.bk - 1) / lc.bk * lc.bk;
      run_live(i, lc, dyn != 0);
    }
  return 0;
}
