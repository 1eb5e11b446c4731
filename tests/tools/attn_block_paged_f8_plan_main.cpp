// Program of tests/test_attn_block_paged_f8_plan.py: attn_block_paged_f8_plan (neural-speed_amd/csrc/ns_attn_plan.cpp) beside attn_block_paged_plan of the
// same shape.  Host code only.  Lines:
//   plan   <the call> | <the fields of the FP8 plan> | <the fields of the fp16 plan>
//   refuse what=.. | <the fields of the FP8 plan>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;

struct Case {
  int hs = 128, cap = 2048, hn = 8, hkv = 8, bs = 2, bk = 16, max_q = 16, head_major = 0;
  long long block_step = 0;  // 0: a block's own size
  long long step_sl = 0, step_head = 0;  // 0: by the layout
  uintptr_t vbase = 0x200000;
  float k_sc = 0.25f, v_sc = 2.f;
  bool null_table = false;
  int pool_blocks = 0;  // 0: the table's blocks + 4
};
static const int g_lens[64] = {0}, g_start[65] = {0};
static const int g_table[1] = {0};  // (only its address is used by a plan)

static AttnBlockPagedPlan plan(const Case& c, bool f8, std::string* why) {
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = reinterpret_cast<float*>(uintptr_t(0x10000));
  a.K = reinterpret_cast<decltype(a.K)>(uintptr_t(0x100000));
  a.V = reinterpret_cast<decltype(a.V)>(c.vbase);
  a.dst = reinterpret_cast<float*>(uintptr_t(0x300000));
  a.Q_sc = 0.5f, a.dst_sc = 4.f, a.K_sc = c.k_sc, a.V_sc = c.v_sc;
  a.QK_scale = 0.125f;
  a.attn_flags = NS_ATTN_FLAG_IS_CAUSAL;
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = c.max_q, a.sl_kv = c.cap;
  a.Q_layout = a.K_layout = a.V_layout = a.dst_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.step_q_head_num = a.step_dst_head_num = c.hs;
  a.step_q_sl = a.step_dst_sl = c.hn * c.hs;
  a.step_k_head_size = a.step_v_head_size = 1;
  a.step_k_sl = a.step_v_sl = c.step_sl ? c.step_sl : (c.head_major ? c.hs : c.hkv * c.hs);
  a.step_k_head_num = a.step_v_head_num = c.step_head ? c.step_head : (c.head_major ? (long long)c.bk * c.hs : c.hs);
  AttnPage pg;
  pg.table = c.null_table ? nullptr : g_table;
  pg.block_shift = attn_block_shift(c.bk);
  pg.table_stride = c.cap / c.bk;
  pg.pool_blocks = c.pool_blocks ? c.pool_blocks : pg.table_stride * c.bs + 4;
  pg.block_step = c.block_step ? c.block_step : (long long)c.bk * c.hkv * c.hs;
  return f8 ? attn_block_paged_f8_plan(a, nullptr, AttnKnobs(), pg, g_start, g_lens, 1, why)
            : attn_block_paged_plan(a, nullptr, AttnKnobs(), pg, g_start, g_lens, 1, why);
}

static void print_fields(const AttnBlockPagedPlan& pl, const std::string& why) {
  const AttnSplitParams& sp = pl.pp.sp;
  const AttnParams& p = sp.a;
  printf("ok=%d f8=%d hs_pad=%d grid=%u,%u,%u block=%u mgrid=%u,%u,%u pbytes=%zu nsplit=%d kps=%d gfull=%d dyn=%d kmove=%d kdelta=%d qstart=%d "
         "table=%d ts=%d shift=%d blocks=%d bstep=%lld k=%llx v=%llx q=%llx dst=%llx slq=%d slkv=%d hn=%d hkv=%d hs=%d flags=%u ksl=%lld khead=%lld "
         "vsl=%lld vhead=%lld kbs=%lld qbs=%lld qsl=%lld qhead=%lld dsl=%lld dhead=%lld qk=%a out=%a why=%s",
         int(pl.ok), int(pl.f8), pl.hs_pad, pl.grid.x, pl.grid.y, pl.grid.z, pl.block.x, pl.merge_grid.x, pl.merge_grid.y, pl.merge_grid.z, pl.partial_bytes,
         sp.nsplit, sp.keys_per_split, sp.g_full, sp.dyn_min_keys, sp.kmove == g_lens, sp.kdelta, pl.pp.q_start == g_start, pl.pp.pg.table == g_table,
         pl.pp.pg.table_stride, pl.pp.pg.block_shift, pl.pp.pg.pool_blocks, pl.pp.pg.block_step, (unsigned long long)uintptr_t(p.k),
         (unsigned long long)uintptr_t(p.v), (unsigned long long)uintptr_t(p.q), (unsigned long long)uintptr_t(p.dst), p.sl_q, p.sl_kv, p.head_num,
         p.heads_kv, p.head_size, p.flags, p.step_k_sl, p.step_k_head_num, p.step_v_sl, p.step_v_head_num, p.step_k_bs, p.step_q_bs, p.step_q_sl,
         p.step_q_head_num, p.step_dst_sl, p.step_dst_head_num, p.qk_scale, p.out_scale, why.c_str());
}
static void run(const char* kind, const char* what, const Case& c, bool both) {
  std::string why8, why16;
  printf("%s what=%s hs=%d cap=%d hn=%d hkv=%d bs=%d bk=%d max_q=%d hm=%d | ", kind, what, c.hs, c.cap, c.hn, c.hkv, c.bs, c.bk, c.max_q, c.head_major);
  print_fields(plan(c, true, &why8), why8);
  if (both) {
    printf(" | ");
    print_fields(plan(c, false, &why16), why16);
  }
  printf("\n");
}

int main(int argc, char** argv) {
  // far hs bk cap requests max_q pool_blocks block_step step_sl step_head: the pool of the far-address test (4 / 2 heads), whose numbers
  // (tests/tools/attn_far_layout.py) the caller passes -> a plan line with what=far
  if (argc == 11 && std::string(argv[1]) == "far") {
    const auto at = [&](int i) { return atoll(argv[i]); };
    Case c;
    c.hn = 4, c.hkv = 2, c.hs = int(at(2)), c.bk = int(at(3)), c.cap = int(at(4)), c.bs = int(at(5)), c.max_q = int(at(6)), c.pool_blocks = int(at(7));
    c.block_step = at(8), c.step_sl = at(9), c.step_head = at(10);
    run("plan", "far", c, true);
    return 0;
  }
  const int groups[][2] = {{8, 8}, {8, 2}, {8, 1}};
  int n = 0;
  for (int bk : {16, 64, 256})
    for (int bs : {1, 3, 33})
      for (const auto& g : groups)
        for (int hs : {64, 128})
          for (int max_q : {1, 16, 127})
            for (int cap : {256, 1000, 8192}) {
              Case c;
              c.bs = bs, c.hn = g[0], c.hkv = g[1], c.hs = hs, c.bk = bk, c.max_q = max_q, c.cap = (cap + bk - 1) / bk * bk, c.head_major = n++ & 1;
              run("plan", "grid", c, true);
            }
  Case c;
  run("refuse", "none", c, false);
  c = Case(), c.hs = 72;
  run("refuse", "head_size", c, false);
  c = Case(), c.step_sl = 8 * 128 + 8, c.block_step = 16 * (8 * 128 + 8);
  run("refuse", "step_sl", c, false);
  c = Case(), c.step_head = 128 + 8, c.step_sl = 8 * (128 + 8), c.block_step = 16 * 8 * (128 + 8);
  run("refuse", "step_head", c, false);
  c = Case(), c.block_step = 16 * 8 * 128 + 8;
  run("refuse", "block_step", c, false);
  c = Case(), c.vbase = 0x200008;
  run("refuse", "base", c, false);
  c = Case(), c.k_sc = 0.f;
  run("refuse", "k_scale_zero", c, false);
  c = Case(), c.v_sc = -1.f;
  run("refuse", "v_scale_negative", c, false);
  c = Case(), c.v_sc = std::numeric_limits<float>::infinity();
  run("refuse", "v_scale_inf", c, false);
  c = Case(), c.k_sc = std::numeric_limits<float>::quiet_NaN();
  run("refuse", "k_scale_nan", c, false);
  c = Case(), c.hs = 80;  // (a legal FP8 pool; the block entry's own refusal)
  run("refuse", "head_size_80", c, false);
  c = Case(), c.null_table = true;
  run("refuse", "null_table", c, false);
  return 0;
}
